"""What the walk benchmarks tools/bench_{kdtree,rbsp,rbspkd,bsppaper}.py share: the scenes (killeroo-simple and the atrium
stand-in of tools/scene_gen.py), the ray sets — camera rays (closest hit, 700x700 x 4 samples, tile order) and shadow rays from
their hit points to a point above the scene's centre (any hit) — resident in HBM with their output buffers for
hprt_intersect_device / hprt_occluded_device, and the event timers.  DESIGN.md §8a-§8d quote figures measured on these rays."""
import importlib, os, sys, tempfile
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
hprt = importlib.import_module("thesis-pbrt-v3_amd")
import orc
import scene_gen

KILLEROO = os.path.join(ROOT, "tests", "golden", "killeroo_simple.hprt")
dev = torch.device("cuda", 0)


def scene_model(name):
    """(model, baked file) of killeroo-simple or the atrium stand-in"""
    if name == "killeroo-simple":
        return hprt.Model.load(KILLEROO), KILLEROO
    d = tempfile.mkdtemp(prefix="hprt_walk_")
    p = os.path.join(d, "atrium.pbrt")
    open(p, "w").write(scene_gen.atrium(1.0)[0])
    m = hprt.Model.parse(p)
    baked = os.path.join(d, "atrium.hprt")
    m.save(baked)
    return m, baked


def camera_rays(baked):
    """(o, d) of the scene's camera rays, 700x700 x 4 samples, 16x16 tiles in row order, sample by sample"""
    px, py = [], []
    for ty in range(44):
        for tx in range(44):
            X, Y = np.meshgrid(np.arange(tx * 16, min(tx * 16 + 16, 700)), np.arange(ty * 16, min(ty * 16 + 16, 700)))
            px.append(X.ravel()); py.append(Y.ravel())
    px = np.tile(np.concatenate(px).astype(np.int32), 4); py = np.tile(np.concatenate(py).astype(np.int32), 4)
    s = np.repeat(np.arange(4), px.shape[0] // 4).astype(np.int64)
    return orc.OracleScene(baked).camera_rays(px, py, s)


def shadow_rays(o, d, t, prim):
    """(origin, direction, tMax) of the rays from the hit points (t, prim of the rays o, d) to a point above the scene's centre"""
    hitm = prim >= 0
    p = (o + d * np.where(np.isfinite(t), t, 0)[:, None]).astype(np.float32)[hitm]
    light = np.array([np.mean(p[:, 0]), np.mean(p[:, 1]), np.max(p[:, 2]) + 1.0], np.float32)
    sd = (light - p).astype(np.float32)
    so = p + sd * np.float32(1e-4)
    return so, sd, np.full(so.shape[0], 1 - 1e-4, np.float32)


def to7(o, d, tmax):
    return torch.from_numpy(np.concatenate([o.T, d.T, tmax[None]], 0).astype(np.float32).copy()).to(dev)


class RaySets:
    """The n camera rays of a baked scene and the ns shadow rays from the hits `hit_scene` finds for them, on the device with
    the output buffers; closest(scene) and any(scene) walk them through a scene's device entry points."""

    def __init__(self, baked, hit_scene):
        self.o, self.d = camera_rays(baked)
        self.n = self.o.shape[0]
        self.inf = np.full(self.n, np.inf, np.float32)
        t, self.prim, _ = hit_scene.intersect(self.o, self.d, self.inf)
        so, sd, stm = shadow_rays(self.o, self.d, t, self.prim)
        self.ns = so.shape[0]
        self.R = to7(self.o, self.d, self.inf); self.S = to7(so, sd, stm)
        self.tt = torch.empty(self.n, dtype=torch.float32, device=dev); self.pp = torch.empty(self.n, dtype=torch.int32, device=dev)
        self.bb = torch.empty(3 * self.n, dtype=torch.float32, device=dev); self.occ = torch.empty(self.ns, dtype=torch.uint8, device=dev)

    def closest(self, sc):
        sc.intersect_device(self.n, self.R.data_ptr(), self.tt.data_ptr(), self.pp.data_ptr(), self.bb.data_ptr())

    def any(self, sc):
        sc.occluded_device(self.ns, self.S.data_ptr(), self.occ.data_ptr())


def once(fn):
    """milliseconds of one call"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def timed(fn, iters):
    """milliseconds of the best of `iters` calls after one warm-up call"""
    fn(); torch.cuda.synchronize()
    return min(once(fn) for _ in range(iters))
