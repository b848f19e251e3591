"""Accelerator "bvhold" beside the fork's BVH: build seconds (best of `iters`) of hprt_bvh_build, of the four host split methods of
hprt_bvhold_build and of the device HLBVH build (hprt_bvhold_build_device), with nodes, leaves and depth, and the closest-hit and
any-hit Grays/s of k_walk4 over each tree (tools/walk_bench.py's ray sets: camera rays, and shadow rays from their hit points).
Scenes: killeroo-simple and the atrium stand-in (tools/scene_gen.py), in one process.  Prints one JSON line per scene; DESIGN.md
§8q quotes them.  No figure here is a pass condition of anything.
usage: python tools/bench_bvhold.py [iters]"""
import json, sys, time
import numpy as np
import walk_bench as wb
from walk_bench import hprt

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 5


def best(make):
    """(the tree of the last call, seconds of the best of `iters` calls)"""
    secs = []
    for _ in range(iters):
        t = time.perf_counter()
        tree = make()
        secs.append(time.perf_counter() - t)
    return tree, min(secs)


for name in ("killeroo-simple", "atrium"):
    m, baked = wb.scene_model(name)
    builds = [("bvh", lambda: hprt.Bvh(m))]
    builds += [("bvhold_" + sm, lambda sm=sm: hprt.BvhOld(m, split_method=sm)) for sm in ("sah", "hlbvh", "middle", "equal")]
    builds += [("bvhold_hlbvh_device", lambda: hprt.BvhOld(m, split_method="hlbvh", device=0))]
    res, rays, trees = {}, None, {}
    for label, make in builds:
        if label.endswith("_device"):
            make()      # (the first call loads the code object)
        tree, sec = best(make)
        trees[label] = tree
        i = tree.info()
        r = {"build_s": round(sec, 4), "nodes": i["nodes"], "leaves": i["leaves"], "depth": i["max_depth"]}
        if tree.__dict__.get("build_stats"):
            st = tree.build_stats
            r.update(device_s=round(st["seconds_device"], 4), treelets=st["treelets"], treelets_host=st["treelets_host"], launches=st["launches"])
        sc = hprt.Scene(m, tree, device=0)
        if rays is None:
            rays = wb.RaySets(baked, sc)
            res["closest_rays"], res["any_rays"] = rays.n, rays.ns
        r["closest_grays"] = round(rays.n / wb.timed(lambda: rays.closest(sc), iters) / 1e6, 3)
        r["any_grays"] = round(rays.ns / wb.timed(lambda: rays.any(sc), iters) / 1e6, 3)
        res[label] = r
    a, b = trees["bvhold_hlbvh"].arrays(), trees["bvhold_hlbvh_device"].arrays()
    res["device_tree_equals_host_tree"] = bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))
    print(json.dumps({name: res}), flush=True)
