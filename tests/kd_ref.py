"""ctypes wrapper around tests/kd_reference.cpp, the test-side restatement of the fork's kd-tree (build and both walks over the
oracle's primitive tests).  Compiled with g++ into a per-process temporary directory on first use — test infrastructure only."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_lib = None


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="kdref"), "libkdref.so")
        cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function",
               "-I", os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests", "kd_reference.cpp"), "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("kd_reference.cpp failed to build:\n" + r.stderr)
        L = C.CDLL(out)
        vp, sz, u32p = C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)
        L.kdref_last_error.restype = C.c_char_p
        L.kdref_build.restype = vp
        L.kdref_build.argtypes = [sz, vp, vp, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, u32p]
        L.kdref_copy.argtypes = [vp, vp, vp]
        L.kdref_free.argtypes = [vp]
        L.kdref_scene_load.restype = vp
        L.kdref_scene_load.argtypes = [C.c_char_p]
        L.kdref_scene_free.argtypes = [vp]
        L.kdref_scene_prims.restype = sz
        L.kdref_scene_prims.argtypes = [vp]
        L.kdref_scene_bounds.argtypes = [vp, vp, vp]
        L.kdref_scene_tree.argtypes = [vp, u32p, vp, vp]
        L.kdref_scene_splits.restype = sz
        L.kdref_scene_splits.argtypes = [vp, vp, vp, sz]
        L.kdref_intersect.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, vp]
        L.kdref_occluded.argtypes = [vp, sz, vp, vp, vp, vp, vp]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def build(bmin, bmax, isect_cost=80, trav_cost=1, empty_bonus=0.0, max_prims=1, max_depth=-1):
    """(nodes [n, 2] uint32, primitiveIndices) of the restated KdTreeAccel::buildTree."""
    bmin = np.ascontiguousarray(bmin, np.float32); bmax = np.ascontiguousarray(bmax, np.float32)
    sizes = (C.c_uint32 * 2)()
    h = lib().kdref_build(bmin.shape[0], _p(bmin), _p(bmax), isect_cost, trav_cost, empty_bonus, max_prims, max_depth, sizes)
    nodes = np.zeros((sizes[0], 2), np.uint32); idx = np.zeros(max(1, sizes[1]), np.uint32)
    lib().kdref_copy(h, _p(nodes), _p(idx))
    lib().kdref_free(h)
    return nodes, idx[:sizes[1]]


class KdScene:
    """A baked scene with the default kd-tree (intersectcost 80, traversalcost 1, emptybonus 0, maxprims 1, maxdepth -1)."""

    def __init__(self, path):
        self._h = lib().kdref_scene_load(path.encode())
        if not self._h:
            raise RuntimeError(lib().kdref_last_error().decode())
        self.n = lib().kdref_scene_prims(self._h)

    def bounds(self):
        lo = np.zeros((self.n, 3), np.float32); hi = np.zeros((self.n, 3), np.float32)
        lib().kdref_scene_bounds(self._h, _p(lo), _p(hi))
        return lo, hi

    def tree(self):
        sizes = (C.c_uint32 * 2)()
        lib().kdref_scene_tree(self._h, sizes, None, None)
        nodes = np.zeros((sizes[0], 2), np.uint32); idx = np.zeros(max(1, sizes[1]), np.uint32)
        lib().kdref_scene_tree(self._h, sizes, _p(nodes), _p(idx))
        return nodes, idx[:sizes[1]]

    def splits(self, cap=4096):
        ax = np.zeros(cap, np.int32); pos = np.zeros(cap, np.float32)
        k = lib().kdref_scene_splits(self._h, _p(ax), _p(pos), cap)
        return ax[:k], pos[:k]

    def intersect(self, o, d, tmax):
        o = np.ascontiguousarray(o, np.float32); d = np.ascontiguousarray(d, np.float32); tmax = np.ascontiguousarray(tmax, np.float32)
        n = tmax.shape[0]
        t = np.zeros(n, np.float32); prim = np.zeros(n, np.int32); bary = np.zeros((n, 3), np.float32); c = np.zeros((n, 4), np.uint64)
        lib().kdref_intersect(self._h, n, _p(o), _p(d), _p(tmax), _p(t), _p(prim), _p(bary), _p(c))
        return t, prim, bary, c

    def occluded(self, o, d, tmax):
        o = np.ascontiguousarray(o, np.float32); d = np.ascontiguousarray(d, np.float32); tmax = np.ascontiguousarray(tmax, np.float32)
        n = tmax.shape[0]
        occ = np.zeros(n, np.uint8); c = np.zeros((n, 4), np.uint64)
        lib().kdref_occluded(self._h, n, _p(o), _p(d), _p(tmax), _p(occ), _p(c))
        return occ, c

    def __del__(self):
        if getattr(self, "_h", None):
            lib().kdref_scene_free(self._h)
            self._h = None
