"""Build time of an RBSP tree on the host (hprt_rbsp_build, 16 threads) beside the device-assisted build (hprt_rbsp_build_device:
the split candidates of large nodes costed by k_kdopcost), in one process, best of `reps`.  Checks that both trees are the same
bytes.  Prints one JSON line per (scene, M, min_candidates): wall seconds of both, seconds_device, and how nodes and candidates
split between host and device.  DESIGN.md §8i quotes them.
usage: python tools/bench_rbsp_build.py <scene: killeroo-simple | atrium> <M, comma-separated> [reps, default 3] [min_candidates, comma-separated, default 0 = the library's]
  e.g.  bench_rbsp_build.py killeroo-simple 3,7,9,13        the table
        bench_rbsp_build.py killeroo-simple 13 3 256,1024,4096,16384   the threshold sweep
        bench_rbsp_build.py atrium 3   /   bench_rbsp_build.py atrium 13 1    (a step of its own, under its own time limit)"""
import json, sys, time
import numpy as np
import walk_bench as wb
from walk_bench import hprt

name = sys.argv[1]
dirs = [int(x) for x in sys.argv[2].split(",")]
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
mins = [int(x) for x in sys.argv[4].split(",")] if len(sys.argv) > 4 else [0]
m, _ = wb.scene_model(name)
for M in dirs:
    host_s, host = [], None
    for _ in range(reps):
        t0 = time.time(); host = hprt.Rbsp(m, n_directions=M, threads=16); host_s.append(time.time() - t0)
    hn, hi = host.arrays()
    for mc in mins:
        dev_s, st = [], None
        for _ in range(reps):
            t0 = time.time(); dev = hprt.Rbsp(m, n_directions=M, threads=16, device=0, min_candidates=mc); dev_s.append(time.time() - t0)
            st = dev.build_stats
        dn, di = dev.arrays()
        print(json.dumps({"scene": name, "M": M, "min_candidates": mc, "host_s": round(min(host_s), 2), "device_s": round(min(dev_s), 2),
                          "same_bytes": bool(np.array_equal(hn, dn) and np.array_equal(hi, di)), "nodes": int(hn.shape[0]),
                          **{k: (round(v, 2) if isinstance(v, float) else v) for k, v in st.items()}}), flush=True)
