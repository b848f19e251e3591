"""Rays per second of the general BSP walk (k_bsppaperwalk, Accelerator "bsppaper") beside the RBSP walk at M = 13 (k_rbspwalk),
the kd walk (k_kdwalk) and the BVH walk plain traces take (k_walk4), with the host build times and tree sizes, on HBM-resident rays
through hprt_intersect_device / hprt_occluded_device.  The ray sets are tools/bench_rbsp.py's: camera rays (closest hit, 700x700 x
4 samples, tile order) and shadow rays from their hit points to a point above the scene's centre (any hit).  Scenes:
killeroo-simple, and the atrium stand-in when asked for.  Prints one JSON line per scene and walk; DESIGN.md §8d quotes them.
HPRT_LIB=<a build_variant.sh library> measures a variant (the A/B of the axis fetch: -DHPRT_BSPPAPER_LATE_AXIS=1).
usage: python tools/bench_bsppaper.py [iters] [scenes, comma-separated, default killeroo-simple] [bsppaper only: 1]"""
import json, os, sys, time
import walk_bench as wb
from walk_bench import hprt

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 5
scenes = sys.argv[2].split(",") if len(sys.argv) > 2 else ["killeroo-simple"]
only = len(sys.argv) > 3 and sys.argv[3] == "1"

for name in scenes:
    m, baked = wb.scene_model(name)
    bvh_scene = hprt.Scene(m, hprt.Bvh(m), device=0)
    rays = wb.RaySets(baked, bvh_scene)
    walks = []
    if not only:
        walks.append(("walk4", bvh_scene, {}))
        t0 = time.time(); kd = hprt.KdTree(m); kd_s = time.time() - t0
        kd_scene = hprt.Scene(m, hprt.Bvh(m), device=0); kd_scene.attach_kdtree(kd)
        walks.append(("kd", kd_scene, {"build_s": round(kd_s, 2), "nodes": kd.info()["nodes"], "depth": kd.info()["depth"]}))
        t0 = time.time(); rb = hprt.Rbsp(m, n_directions=13); rb_s = time.time() - t0
        sc = hprt.Scene(m, hprt.Bvh(m), device=0); sc.attach_rbsp(rb)
        walks.append(("rbsp-13", sc, {"build_s": round(rb_s, 2), "nodes": rb.info()["nodes"], "depth": rb.info()["depth"]}))
    t0 = time.time(); bp = hprt.BspPaper(m, isect_cost=80, threads=16); bp_s = time.time() - t0
    print(json.dumps({"scene": name, "bsppaper_build_s": round(bp_s, 2), **bp.info()}), flush=True)
    sc = hprt.Scene(m, hprt.Bvh(m), device=0); sc.attach_bsppaper(bp)
    walks.append(("bsppaper", sc, {"build_s": round(bp_s, 2), "nodes": bp.info()["nodes"], "depth": bp.info()["depth"],
                                   "lib": os.path.basename(hprt.LIB_PATH)}))
    for label, sc, extra in walks:
        mc = wb.timed(lambda: rays.closest(sc), iters)
        ma = wb.timed(lambda: rays.any(sc), iters)
        res = dict(extra, closest_rays=rays.n, any_rays=rays.ns, closest_grays=round(rays.n / mc / 1e6, 3), any_grays=round(rays.ns / ma / 1e6, 3))
        print(json.dumps({"scene": name, "walk": label, **res}), flush=True)
