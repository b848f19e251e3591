"""rbsp-M against rbspkd-M on killeroo-simple, M = 3, 7, 9, 13 — the thesis' comparison — in one session: per tree the nodes,
depth and kd / oblique share of the interior nodes, the host build time on 16 threads, and closest- / any-hit rays per second
of k_rbspwalk and k_rbspkdwalk, the two walks alternated and the best of `iters` rounds kept.  The ray sets are
tools/bench_rbsp.py's (camera rays, 700x700 x 4 samples in tile order; shadow rays from their hits to a point above the scene).
With --counting, one counting render per tree as the scene file sets it (8 spp) adds the node traversals, split into kd and bsp
interior nodes, and the triangle tests.  Prints one JSON line per tree; DESIGN.md §8c quotes them.
usage: python tools/bench_rbspkd.py [iters] [--counting]"""
import json, sys, time
import walk_bench as wb
from walk_bench import hprt

args = [a for a in sys.argv[1:] if not a.startswith("--")]
iters = int(args[0]) if args else 5
counting = "--counting" in sys.argv

m, baked = wb.scene_model("killeroo-simple")
rays = wb.RaySets(baked, hprt.Scene(m, hprt.Bvh(m), device=0))
opt = m.options.copy(); opt.spp = 8
keys = ("rays", "shadow_rays", "nodes_fetched", "nodes_fetched_p", "nodes_entered", "nodes_entered_p", "tri_tests", "tri_tests_p")

for M in (3, 7, 9, 13):
    walks = []
    for kind in ("rbsp", "rbspkd"):
        t0 = time.time()
        tree = hprt.Rbsp(m, n_directions=M, threads=16) if kind == "rbsp" else hprt.RbspKd(m, n_directions=M, threads=16)
        build_s = time.time() - t0
        sc = hprt.Scene(m, hprt.Bvh(m), device=0)
        (sc.attach_rbsp if kind == "rbsp" else sc.attach_rbspkd)(tree)
        nodes, _ = tree.arrays()
        ax = nodes[:, 1] & ((1 << M.bit_length()) - 1)
        kd, bsp = int((ax < 3).sum()), int(((ax >= 3) & (ax != M)).sum())
        info = tree.info()
        walks.append(["%s-%d" % (kind, M), sc, {"nodes": info["nodes"], "depth": info["depth"], "kd_interior": kd, "bsp_interior": bsp,
                                               "kd_share": round(kd / max(1, kd + bsp), 3), "build_s": round(build_s, 2)}, 1e30, 1e30])
    for w in walks:                        # warm-up
        wb.once(lambda: rays.closest(w[1]))
        wb.once(lambda: rays.any(w[1]))
    for _ in range(iters):                 # the two walks alternated
        for w in walks:
            w[3] = min(w[3], wb.once(lambda: rays.closest(w[1])))
            w[4] = min(w[4], wb.once(lambda: rays.any(w[1])))
    for label, sc, extra, mc, ma in walks:
        res = dict(extra, closest_grays=round(rays.n / mc / 1e6, 3), any_grays=round(rays.ns / ma / 1e6, 3))
        if counting:
            _, st = sc.render(opt, count_work=True)
            res.update({k: int(st[k]) for k in keys})
            kdc = sc.kd_counters() if label.startswith("rbspkd") else (0, 0)
            res.update(kd_nodes=kdc[0], kd_nodes_p=kdc[1], bsp_nodes=int(st["nodes_entered"]) - kdc[0], bsp_nodes_p=int(st["nodes_entered_p"]) - kdc[1])
        print(json.dumps({"scene": "killeroo-simple", "tree": label, "closest_rays": rays.n, "any_rays": rays.ns, **res}), flush=True)
