"""rbsp-M against rbspkd-M on killeroo-simple, M = 3, 7, 9, 13 — the thesis' comparison — in one session: per tree the nodes,
depth and kd / oblique share of the interior nodes, the host build time on 16 threads, and closest- / any-hit rays per second
of k_rbspwalk and k_rbspkdwalk, the two walks alternated and the best of `iters` rounds kept.  The ray sets are
tools/bench_rbsp.py's (camera rays, 700x700 x 4 samples in tile order; shadow rays from their hits to a point above the scene).
With --counting, one counting render per tree as the scene file sets it (8 spp) adds the node traversals, split into kd and bsp
interior nodes, and the triangle tests.  Prints one JSON line per tree; DESIGN.md §8c quotes them.
usage: python tools/bench_rbspkd.py [iters] [--counting]"""
import importlib, json, os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
hprt = importlib.import_module("thesis-pbrt-v3_amd")
import orc

args = [a for a in sys.argv[1:] if not a.startswith("--")]
iters = int(args[0]) if args else 5
counting = "--counting" in sys.argv
dev = torch.device("cuda", 0)


def to7(o, d, tmax):
    return torch.from_numpy(np.concatenate([o.T, d.T, tmax[None]], 0).astype(np.float32).copy()).to(dev)


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


path = os.path.join(ROOT, "tests", "golden", "killeroo_simple.hprt")
m = hprt.Model.load(path)
oracle = orc.OracleScene(path)
px, py = [], []
for ty in range(44):
    for tx in range(44):
        X, Y = np.meshgrid(np.arange(tx * 16, min(tx * 16 + 16, 700)), np.arange(ty * 16, min(ty * 16 + 16, 700)))
        px.append(X.ravel()); py.append(Y.ravel())
px = np.tile(np.concatenate(px).astype(np.int32), 4); py = np.tile(np.concatenate(py).astype(np.int32), 4)
s = np.repeat(np.arange(4), px.shape[0] // 4).astype(np.int64)
o, d = oracle.camera_rays(px, py, s)
n = o.shape[0]
inf = np.full(n, np.inf, np.float32)
t, prim, _ = hprt.Scene(m, hprt.Bvh(m), device=0).intersect(o, d, inf)
hitm = prim >= 0
p = (o + d * np.where(np.isfinite(t), t, 0)[:, None]).astype(np.float32)[hitm]
light = np.array([np.mean(p[:, 0]), np.mean(p[:, 1]), np.max(p[:, 2]) + 1.0], np.float32)
sd = (light - p).astype(np.float32)
so = p + sd * np.float32(1e-4)
stm = np.full(so.shape[0], 1 - 1e-4, np.float32)
R = to7(o, d, inf); S = to7(so, sd, stm)
ns = so.shape[0]
tt = torch.empty(n, dtype=torch.float32, device=dev); pp = torch.empty(n, dtype=torch.int32, device=dev)
bb = torch.empty(3 * n, dtype=torch.float32, device=dev); occ = torch.empty(ns, dtype=torch.uint8, device=dev)
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
        once(lambda: w[1].intersect_device(n, R.data_ptr(), tt.data_ptr(), pp.data_ptr(), bb.data_ptr()))
        once(lambda: w[1].occluded_device(ns, S.data_ptr(), occ.data_ptr()))
    for _ in range(iters):                 # the two walks alternated
        for w in walks:
            w[3] = min(w[3], once(lambda: w[1].intersect_device(n, R.data_ptr(), tt.data_ptr(), pp.data_ptr(), bb.data_ptr())))
            w[4] = min(w[4], once(lambda: w[1].occluded_device(ns, S.data_ptr(), occ.data_ptr())))
    for label, sc, extra, mc, ma in walks:
        res = dict(extra, closest_grays=round(n / mc / 1e6, 3), any_grays=round(ns / ma / 1e6, 3))
        if counting:
            _, st = sc.render(opt, count_work=True)
            res.update({k: int(st[k]) for k in keys})
            kdc = sc.kd_counters() if label.startswith("rbspkd") else (0, 0)
            res.update(kd_nodes=kdc[0], kd_nodes_p=kdc[1], bsp_nodes=int(st["nodes_entered"]) - kdc[0], bsp_nodes_p=int(st["nodes_entered_p"]) - kdc[1])
        print(json.dumps({"scene": "killeroo-simple", "tree": label, "closest_rays": n, "any_rays": ns, **res}), flush=True)
