"""Build time of a node-based BSP tree on the host (hprt_bspnode_build / hprt_bspnodekd_build, 16 threads) beside the device-assisted
build (hprt_bspnode_build_device / hprt_bspnodekd_build_device: the split candidates of large nodes costed by k_sweepcost), in one
process, best of `reps`.  Checks that both trees are the same bytes.  Prints one JSON line per (scene, tree, min_candidates): wall
seconds of both, seconds_device, and how nodes and candidates split between host and device.  The yardstick is always the host
entry, never the device build against itself.  DESIGN.md §8o quotes the lines.
usage: python tools/bench_bspnode_build.py <scene: killeroo-simple | atrium> [reps, default 1] [min_candidates, comma-separated,
                                           default 256,1024,4096,16384] [trees, comma-separated, default
                                           bspclusterfastkd,bsparbitraryfastkd,bsprandom,bspcluster] [K, default 5] [seed, default 5489]
  e.g.  bench_bspnode_build.py killeroo-simple                          the table with the threshold sweep
        bench_bspnode_build.py killeroo-simple 1 0 bsprandom             one host build, one device build at the library's threshold"""
import json, sys, time
import numpy as np
import walk_bench as wb
from walk_bench import hprt

name = sys.argv[1]
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 1
mins = [int(x) for x in sys.argv[3].split(",")] if len(sys.argv) > 3 else [256, 1024, 4096, 16384]
trees = sys.argv[4].split(",") if len(sys.argv) > 4 else ["bspclusterfastkd", "bsparbitraryfastkd", "bsprandom", "bspcluster"]
K = int(sys.argv[5]) if len(sys.argv) > 5 else 5
seed = int(sys.argv[6]) if len(sys.argv) > 6 else hprt.BSPNODE_DEFAULT_SEED
m, _ = wb.scene_model(name)
for tree in trees:
    cls = hprt.BspNodeKd if tree.endswith("fastkd") else hprt.BspNode
    host_s, host = [], None
    for _ in range(reps):
        t0 = time.time(); host = cls(m, tree, n_directions=K, seed=seed, threads=16); host_s.append(time.time() - t0)
    hn, hi = host.arrays()
    for mc in mins:
        dev_s, st = [], None
        for _ in range(reps):
            t0 = time.time(); dev = cls(m, tree, n_directions=K, seed=seed, threads=16, device=0, min_candidates=mc); dev_s.append(time.time() - t0)
            st = dev.build_stats
        dn, di = dev.arrays()
        print(json.dumps({"scene": name, "tree": "%s-%d" % (tree, K), "min_candidates": mc, "host_s": round(min(host_s), 2), "device_s": round(min(dev_s), 2),
                          "same_bytes": bool(np.array_equal(hn, dn) and np.array_equal(hi, di)), "nodes": int(hn.shape[0]),
                          **{k: (round(v, 2) if isinstance(v, float) else v) for k, v in st.items()}}), flush=True)
