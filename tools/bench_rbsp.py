"""Rays per second of the RBSP walk (k_rbspwalk) for M = 3, 7, 9, 13 beside the kd walk (k_kdwalk) and the BVH walk plain traces
take (k_walk4), with the host build times, on HBM-resident rays through hprt_intersect_device / hprt_occluded_device.  The ray
sets are tools/bench_kdtree.py's: camera rays (closest hit, 700x700 x 4 samples, tile order) and shadow rays from their hit
points to a point above the scene's centre (any hit).  Scenes: killeroo-simple (every M) and the atrium stand-in (M = 3 unless
listed).  Prints one JSON line per scene and walk; DESIGN.md §8b quotes them.
usage: python tools/bench_rbsp.py [iters] [atrium directions, comma-separated, default 3]"""
import json, sys, time
import walk_bench as wb
from walk_bench import hprt

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 5
atrium_dirs = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else [3]

for name, dirs in (("killeroo-simple", [3, 7, 9, 13]), ("atrium", atrium_dirs)):
    m, baked = wb.scene_model(name)
    bvh_scene = hprt.Scene(m, hprt.Bvh(m), device=0)
    rays = wb.RaySets(baked, bvh_scene)
    walks = [("walk4", bvh_scene, {})]
    t0 = time.time(); kd = hprt.KdTree(m); kd_s = time.time() - t0
    kd_scene = hprt.Scene(m, hprt.Bvh(m), device=0); kd_scene.attach_kdtree(kd)
    walks.append(("kd", kd_scene, {"build_s": round(kd_s, 2), "nodes": kd.info()["nodes"], "depth": kd.info()["depth"]}))
    for M in dirs:
        t0 = time.time(); rb = hprt.Rbsp(m, n_directions=M); rb_s = time.time() - t0
        sc = hprt.Scene(m, hprt.Bvh(m), device=0); sc.attach_rbsp(rb)
        walks.append(("rbsp-%d" % M, sc, {"build_s": round(rb_s, 2), "nodes": rb.info()["nodes"], "depth": rb.info()["depth"]}))
    for label, sc, extra in walks:
        mc = wb.timed(lambda: rays.closest(sc), iters)
        ma = wb.timed(lambda: rays.any(sc), iters)
        res = dict(extra, closest_rays=rays.n, any_rays=rays.ns, closest_grays=round(rays.n / mc / 1e6, 3), any_grays=round(rays.ns / ma / 1e6, 3))
        print(json.dumps({"scene": name, "walk": label, **res}), flush=True)
