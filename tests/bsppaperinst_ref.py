"""ctypes wrapper around tests/bsppaperinst_reference.cpp, the test-side restatement of an instanced Accelerator "bsppaper" /
"bsppaperkd" scene (two levels of BSP or BSPKd joined by TransformedPrimitive), compiled with g++ into a per-process temporary
directory on first use — test infrastructure only.  The trees are given: BspPaperInstScene.take(handle) copies them out of an
hprt.BspPaperInst; nodes are the reference's 5 words."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_lib = None
_VP, _SZ, _INT = C.c_void_p, C.c_size_t, C.c_int
_SIG = {
    "last_error": (C.c_char_p, []),
    "scene_load": (_VP, [C.c_char_p, _INT]),
    "dot_only": (None, [_VP, _INT]),
    "scene_free": (None, [_VP]),
    "counts": (None, [_VP, _VP]),
    "prims": (_SZ, [_VP, _INT, _VP, _VP, _VP, _VP]),
    "tree_bounds": (None, [_VP, _INT, _VP]),
    "build": (_VP, [_VP, _INT, _INT, _INT, _INT, C.c_float, _INT, _INT, _VP]),
    "built_copy": (None, [_VP, _VP, _VP, _VP]),
    "built_free": (None, [_VP]),
    "set_tree": (None, [_VP, _INT, _SZ, _VP, _SZ, _VP, _VP]),
    "intersect": (None, [_VP, _SZ, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "occluded": (None, [_VP, _SZ, _VP, _VP, _VP, _VP, _VP, _VP]),
}


def _load():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="bspinstref"), "libbspinstref.so")
        cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function",
               "-I", os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests", "bsppaperinst_reference.cpp"), "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("bsppaperinst_reference.cpp failed to build:\n" + r.stderr)
        L = C.CDLL(out)
        for name, (restype, argtypes) in _SIG.items():
            f = getattr(L, "bspinstref_" + name)
            f.restype, f.argtypes = restype, argtypes
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class BspPaperInstScene:
    """A baked scene with object instances, walked over given trees with the general BSP step or (kd_aware) BSPKdNode's.  Hits number the ordered primitives of all aggregates (top level, then object 0, 1, ...), as Scene.intersect_instanced
    does."""

    def __init__(self, path, kd_aware=False):
        self._lib = _load()
        self.kd_aware = bool(kd_aware)
        self._h = self._lib.bspinstref_scene_load(path.encode(), int(self.kd_aware))
        if not self._h:
            raise RuntimeError(self._lib.bspinstref_last_error().decode())
        c = np.zeros(3, np.uint32)
        self._lib.bspinstref_counts(self._h, _p(c))
        self.n_top, self.n_objects, self.n_instances = (int(v) for v in c)

    def prims(self, obj=-1):
        """(is_tri [n] uint8, p9 [n, 9], bmin [n, 3], bmax [n, 3]) of the primitives of the top level (obj < 0: an instance is no
        triangle, its bound TransformedPrimitive::WorldBound) or of one object (in object space), in creation order: what the trees
        are built over"""
        n = self._lib.bspinstref_prims(self._h, obj, None, None, None, None)
        tri = np.zeros(n, np.uint8); p9 = np.zeros((n, 9), np.float32); lo = np.zeros((n, 3), np.float32); hi = np.zeros((n, 3), np.float32)
        self._lib.bspinstref_prims(self._h, obj, _p(tri), _p(p9), _p(lo), _p(hi))
        return tri, p9, lo, hi

    def tree_bounds(self, obj=-1):
        b = np.zeros(6, np.float32)
        self._lib.bspinstref_tree_bounds(self._h, obj, _p(b))
        return b

    def build(self, obj=-1, isect_cost=80, trav_cost=5, kd_trav_cost=1, empty_bonus=0.0, max_prims=1, max_depth=-1):
        """(nodes [n, 5] uint32, prim_indices, bounds [6]) of the test-side Build of tests/bsppaper_reference.cpp (kd_aware:
        BuildKd of tests/bsppaperkd_reference.cpp) over prims(obj)"""
        sizes = np.zeros(2, np.uint32)
        t = self._lib.bspinstref_build(self._h, obj, isect_cost, trav_cost, kd_trav_cost, empty_bonus, max_prims, max_depth, _p(sizes))
        if not t:
            raise RuntimeError(self._lib.bspinstref_last_error().decode())
        nodes = np.zeros((int(sizes[0]), 5), np.uint32); idx = np.zeros(int(sizes[1]), np.uint32); b = np.zeros(6, np.float32)
        self._lib.bspinstref_built_copy(t, _p(nodes), _p(idx), _p(b))
        self._lib.bspinstref_built_free(t)
        return nodes, idx, b

    def set_tree(self, obj, nodes, idx, bounds=None):
        nodes = np.ascontiguousarray(nodes, np.uint32); idx = np.ascontiguousarray(idx, np.uint32)
        assert nodes.ndim == 2 and nodes.shape[1] == 5
        b = None if bounds is None else np.ascontiguousarray(bounds, np.float32)
        self._lib.bspinstref_set_tree(self._h, obj, nodes.shape[0], _p(nodes), idx.shape[0], _p(idx), _p(b))

    def take(self, bspinst):
        """the trees of an hprt.BspPaperInst: the top-level one and every object's"""
        assert bool(bspinst.info()["kd_aware"]) == self.kd_aware
        self.set_tree(-1, *bspinst.copy())
        for o in range(self.n_objects):
            self.set_tree(o, *bspinst.object_copy(o))
        return self

    def dot_only(self, on):
        """the control: a kd-aware scene takes the dot-product step at every interior node, a kd node over the unit axis it names"""
        self._lib.bspinstref_dot_only(self._h, int(bool(on)))

    def intersect(self, o, d, tmax):
        """t, primitive, instance, barycentrics, per ray the counters nodes, interior nodes, leaves, triangle tests, sphere tests, kd
        interior nodes, and the most entries the one todo list held"""
        o = np.ascontiguousarray(o, np.float32); d = np.ascontiguousarray(d, np.float32); tmax = np.ascontiguousarray(tmax, np.float32)
        n = tmax.shape[0]
        t = np.zeros(n, np.float32); prim = np.zeros(n, np.int32); inst = np.zeros(n, np.int32); bary = np.zeros((n, 3), np.float32)
        c = np.zeros((n, 6), np.uint64); todo = np.zeros(n, np.uint32)
        self._lib.bspinstref_intersect(self._h, n, _p(o), _p(d), _p(tmax), _p(t), _p(prim), _p(inst), _p(bary), _p(c), _p(todo))
        return t, prim, inst, bary, c, todo

    def occluded(self, o, d, tmax):
        o = np.ascontiguousarray(o, np.float32); d = np.ascontiguousarray(d, np.float32); tmax = np.ascontiguousarray(tmax, np.float32)
        n = tmax.shape[0]
        occ = np.zeros(n, np.uint8); c = np.zeros((n, 6), np.uint64); todo = np.zeros(n, np.uint32)
        self._lib.bspinstref_occluded(self._h, n, _p(o), _p(d), _p(tmax), _p(occ), _p(c), _p(todo))
        return occ, c, todo

    def __del__(self):
        if getattr(self, "_h", None) and getattr(self, "_lib", None) is not None:
            self._lib.bspinstref_scene_free(self._h)
            self._h = None
