"""Rays per second of the general BSP walk (k_bsppaperwalk, Accelerator "bsppaper") beside the RBSP walk at M = 13 (k_rbspwalk),
the kd walk (k_kdwalk) and the BVH walk plain traces take (k_walk4), with the host build times and tree sizes, on HBM-resident rays
through hprt_intersect_device / hprt_occluded_device.  The ray sets are tools/bench_rbsp.py's: camera rays (closest hit, 700x700 x
4 samples, tile order) and shadow rays from their hit points to a point above the scene's centre (any hit).  Scenes:
killeroo-simple, and the atrium stand-in when asked for.  Prints one JSON line per scene and walk; DESIGN.md §8d quotes them.
HPRT_LIB=<a build_variant.sh library> measures a variant (the A/B of the axis fetch: -DHPRT_BSPPAPER_LATE_AXIS=1).
usage: python tools/bench_bsppaper.py [iters] [scenes, comma-separated, default killeroo-simple] [bsppaper only: 1]"""
import importlib, json, os, sys, tempfile, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
hprt = importlib.import_module("thesis-pbrt-v3_amd")
import orc
import scene_gen

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 5
scenes = sys.argv[2].split(",") if len(sys.argv) > 2 else ["killeroo-simple"]
only = len(sys.argv) > 3 and sys.argv[3] == "1"
dev = torch.device("cuda", 0)


def scene_model(name):
    if name == "killeroo-simple":
        path = os.path.join(ROOT, "tests", "golden", "killeroo_simple.hprt")
        return hprt.Model.load(path), path
    d = tempfile.mkdtemp(prefix="hprt_bsppaper_")
    p = os.path.join(d, "atrium.pbrt")
    open(p, "w").write(scene_gen.atrium(1.0)[0])
    m = hprt.Model.parse(p)
    baked = os.path.join(d, "atrium.hprt")
    m.save(baked)
    return m, baked


def to7(o, d, tmax):
    return torch.from_numpy(np.concatenate([o.T, d.T, tmax[None]], 0).astype(np.float32).copy()).to(dev)


def timed(fn):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e30
    for _ in range(iters):
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1))
    return best


for name in scenes:
    m, baked = scene_model(name)
    oracle = orc.OracleScene(baked)
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
    bvh_scene = hprt.Scene(m, hprt.Bvh(m), device=0)
    t, prim, _ = bvh_scene.intersect(o, d, inf)
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
        mc = timed(lambda: sc.intersect_device(n, R.data_ptr(), tt.data_ptr(), pp.data_ptr(), bb.data_ptr()))
        ma = timed(lambda: sc.occluded_device(ns, S.data_ptr(), occ.data_ptr()))
        res = dict(extra, closest_rays=n, any_rays=ns, closest_grays=round(n / mc / 1e6, 3), any_grays=round(ns / ma / 1e6, 3))
        print(json.dumps({"scene": name, "walk": label, **res}), flush=True)
