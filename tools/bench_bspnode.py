"""Rays per second of the node-based BSP trees (Accelerator "bspclusterfastkd", "bsprandomfastkd", "bsparbitraryfastkd", "bspcluster":
built by csrc/bspnode_builder.cpp with the default seed, walked by k_bsppaperkdwalk / k_bsppaperwalk) beside the kd walk, bsppaperkd
and rbspkd at M = 13, with the host build times on 16 threads, the tree sizes and the kd / plane share of the interior nodes, on
HBM-resident rays through hprt_intersect_device / hprt_occluded_device.  The ray sets are tools/walk_bench.py's: camera rays
(closest hit, 700x700 x 4 samples, tile order) and shadow rays from their hit points to a point above the scene's centre (any hit),
on killeroo-simple.  The walks are alternated and the best of `iters` rounds kept.  With --counting, one counting render per tree
(8 spp) adds the node traversals, split into kd and bsp interior nodes, and the triangle tests.  Prints one JSON line per walk;
DESIGN.md §8f quotes them.
usage: python tools/bench_bspnode.py [iters] [K, default 5] [node-based trees only: 1] [--counting]"""
import json, sys, time
import walk_bench as wb
from walk_bench import hprt

args = [a for a in sys.argv[1:] if not a.startswith("--")]
iters = int(args[0]) if args else 5
K = int(args[1]) if len(args) > 1 else 5
only = len(args) > 2 and args[2] == "1"
counting = "--counting" in sys.argv

m, baked = wb.scene_model("killeroo-simple")
rays = wb.RaySets(baked, hprt.Scene(m, hprt.Bvh(m), device=0))
opt = m.options.copy(); opt.spp = 8
keys = ("rays", "shadow_rays", "nodes_fetched", "nodes_fetched_p", "nodes_entered", "nodes_entered_p", "tri_tests", "tri_tests_p")


def node_based(acc):
    return lambda: hprt.bspnode_tree(m, acc, n_directions=K, threads=16)


builders = [("%s-%d" % (acc, K), node_based(acc)) for acc in ("bspclusterfastkd", "bsprandomfastkd", "bsparbitraryfastkd", "bspcluster")]
if not only:
    builders += [("kd", lambda: (hprt.KdTree(m), "attach_kdtree")), ("bsppaperkd", lambda: (hprt.BspPaperKd(m, isect_cost=80, threads=16), "attach_bsppaperkd")),
                 ("rbspkd-13", lambda: (hprt.RbspKd(m, n_directions=13, threads=16), "attach_rbspkd"))]
walks = []
for label, build in builders:
    t0 = time.time(); tree, attach = build(); build_s = time.time() - t0
    sc = hprt.Scene(m, hprt.Bvh(m), device=0)
    getattr(sc, attach)(tree)
    info = tree.info()
    extra = {"nodes": info["nodes"], "depth": info["depth"], "build_s": round(build_s, 2)}
    kd = info.get("kd_interior", info.get("axis_interior"))
    if kd is not None:
        bsp = info.get("plane_interior", info.get("bsp_interior"))
        extra.update(kd_interior=kd, bsp_interior=bsp, kd_share=round(kd / max(1, kd + bsp), 3))
    print(json.dumps({"tree": label, "built": extra}), flush=True)
    walks.append([label, sc, extra, 1e30, 1e30])
for w in walks:                        # warm-up
    wb.once(lambda: rays.closest(w[1]))
    wb.once(lambda: rays.any(w[1]))
for _ in range(iters):                 # the walks alternated
    for w in walks:
        w[3] = min(w[3], wb.once(lambda: rays.closest(w[1])))
        w[4] = min(w[4], wb.once(lambda: rays.any(w[1])))
for label, sc, extra, mc, ma in walks:
    res = dict(extra, closest_grays=round(rays.n / mc / 1e6, 3), any_grays=round(rays.ns / ma / 1e6, 3))
    if counting:
        _, st = sc.render(opt, count_work=True)
        res.update({k: int(st[k]) for k in keys})
        kdc = sc.kd_counters()
        if label == "kd":
            kdc = (int(st["nodes_entered"]), int(st["nodes_entered_p"]))
        res.update(kd_nodes=kdc[0], kd_nodes_p=kdc[1], bsp_nodes=int(st["nodes_entered"]) - kdc[0], bsp_nodes_p=int(st["nodes_entered_p"]) - kdc[1])
    print(json.dumps({"scene": "killeroo-simple", "walk": label, "closest_rays": rays.n, "any_rays": rays.ns, **res}), flush=True)
