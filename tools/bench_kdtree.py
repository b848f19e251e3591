"""Rays per second of the kd walk (k_kdwalk) beside the BVH walk plain traces take (k_walk4), on HBM-resident rays through
hprt_intersect_device / hprt_occluded_device.  Scenes: killeroo-simple and the atrium stand-in (tools/scene_gen.py).
Ray sets: camera rays (closest hit, 700x700 x 4 samples, tile order) and shadow rays from their hit points to a point above
the scene's centre (any hit).  Prints one JSON line per scene; DESIGN.md quotes them.
usage: python tools/bench_kdtree.py [iters]"""
import json, sys
import walk_bench as wb
from walk_bench import hprt

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 5

for name in ("killeroo-simple", "atrium"):
    m, baked = wb.scene_model(name)
    bvh_scene = hprt.Scene(m, hprt.Bvh(m), device=0)
    kd_scene = hprt.Scene(m, hprt.Bvh(m), device=0)
    tree = hprt.KdTree(m)
    kd_scene.attach_kdtree(tree)
    rays = wb.RaySets(baked, kd_scene)
    res = {"closest_rays": rays.n, "any_rays": rays.ns, "kd_nodes": tree.info()["nodes"], "kd_depth": tree.info()["depth"]}
    for label, sc in (("kd", kd_scene), ("walk4", bvh_scene)):
        mc = wb.timed(lambda: rays.closest(sc), iters)
        ma = wb.timed(lambda: rays.any(sc), iters)
        res[label + "_closest_grays"] = round(rays.n / mc / 1e6, 3)
        res[label + "_any_grays"] = round(rays.ns / ma / 1e6, 3)
    # the two walks answer the same rays the same way up to ties between equally distant hits
    t1, p1, _ = bvh_scene.intersect(rays.o, rays.d, rays.inf)
    res["closest_same_prim_frac"] = float((p1 == rays.prim).mean())
    print(json.dumps({name: res}), flush=True)
