"""ctypes wrapper around tests/bvhold_reference.cpp, the test-side restatement of the stock pbrt-v3 BVH (Accelerator "bvhold":
the four builds, the flattening and the two walks over the oracle's primitive tests).  Compiled with g++ into a per-process
temporary directory on first use — test infrastructure only."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = {"sah": 0, "hlbvh": 1, "middle": 2, "equal": 3}
_lib = None
_VP, _SZ, _INT, _U32P = C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_uint32)
_SIG = {
    "last_error": (C.c_char_p, []),
    "build": (_VP, [_SZ, _VP, _VP, _INT, _INT, _U32P]),
    "copy": (None, [_VP, _VP, _VP]),
    "free": (None, [_VP]),
    "scene_load": (_VP, [C.c_char_p, _INT, _INT]),
    "scene_free": (None, [_VP]),
    "scene_objects": (_SZ, [_VP]),
    "scene_tree": (None, [_VP, _INT, _U32P, _VP, _VP]),
    "scene_bounds": (_SZ, [_VP, _INT, _VP, _VP]),
    "intersect": (None, [_VP, _SZ, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "occluded": (None, [_VP, _SZ, _VP, _VP, _VP, _VP, _VP]),
}


class _Lib:
    def __init__(self):
        out = os.path.join(tempfile.mkdtemp(prefix="bvholdref"), "libbvholdref.so")
        cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function",
               "-I", os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests", "bvhold_reference.cpp"), "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("bvhold_reference.cpp failed to build:\n" + r.stderr)
        L = C.CDLL(out)
        for fn, (restype, argtypes) in _SIG.items():
            f = getattr(L, "bvholdref_" + fn)
            f.restype, f.argtypes = restype, argtypes
            setattr(self, fn, f)


def _load():
    global _lib
    if _lib is None:
        _lib = _Lib()
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _method(m):
    return METHODS[m] if isinstance(m, str) else int(m)


def build(bmin, bmax, split_method="sah", max_node_prims=4):
    """(nodes [n, 8] uint32: the 32-byte LinearBVHNodeOld, orderedPrims) of the restated build; RuntimeError where the reference's
    build stops (a failed check)."""
    L = _load()
    bmin = np.ascontiguousarray(bmin, np.float32).reshape(-1, 3); bmax = np.ascontiguousarray(bmax, np.float32).reshape(-1, 3)
    sizes = (C.c_uint32 * 2)()
    h = L.build(bmin.shape[0], _p(bmin), _p(bmax), _method(split_method), max_node_prims, sizes)
    if not h:
        raise RuntimeError(L.last_error().decode())
    nodes = np.zeros((sizes[0], 8), np.uint32); order = np.zeros(sizes[1], np.uint32)
    L.copy(h, _p(nodes), _p(order))
    L.free(h)
    return nodes, order


class BvhOldScene:
    """A baked scene (with or without object instances) with the restated bvhold trees of every aggregate."""

    def __init__(self, path, split_method="sah", max_node_prims=4):
        self._lib = _load()
        self._h = self._lib.scene_load(path.encode(), _method(split_method), max_node_prims)
        if not self._h:
            raise RuntimeError(self._lib.last_error().decode())
        self.n_objects = self._lib.scene_objects(self._h)

    def tree(self, obj=-1):
        """(nodes, orderedPrims) of the top level (obj < 0) or of object definition obj"""
        sizes = (C.c_uint32 * 2)()
        self._lib.scene_tree(self._h, obj, sizes, None, None)
        nodes = np.zeros((sizes[0], 8), np.uint32); order = np.zeros(sizes[1], np.uint32)
        self._lib.scene_tree(self._h, obj, sizes, _p(nodes), _p(order))
        return nodes, order

    def bounds(self, obj=-1):
        """(bmin, bmax) [n, 3] float32: the world bounds the aggregate's tree is built over, creation order"""
        n = self._lib.scene_bounds(self._h, obj, None, None)
        lo = np.zeros((n, 3), np.float32); hi = np.zeros((n, 3), np.float32)
        self._lib.scene_bounds(self._h, obj, _p(lo), _p(hi))
        return lo, hi

    def intersect(self, o, d, tmax):
        """t, ordered primitive over all aggregates, instance, barycentrics and per ray the counters nodes fetched, nodes entered,
        triangle tests, sphere tests, leaves entered"""
        o = np.ascontiguousarray(o, np.float32); d = np.ascontiguousarray(d, np.float32); tmax = np.ascontiguousarray(tmax, np.float32)
        n = tmax.shape[0]
        t = np.zeros(n, np.float32); prim = np.zeros(n, np.int32); inst = np.zeros(n, np.int32); bary = np.zeros((n, 3), np.float32)
        c = np.zeros((n, 5), np.uint64)
        self._lib.intersect(self._h, n, _p(o), _p(d), _p(tmax), _p(t), _p(prim), _p(inst), _p(bary), _p(c))
        return t, prim, inst, bary, c

    def occluded(self, o, d, tmax):
        o = np.ascontiguousarray(o, np.float32); d = np.ascontiguousarray(d, np.float32); tmax = np.ascontiguousarray(tmax, np.float32)
        n = tmax.shape[0]
        occ = np.zeros(n, np.uint8); c = np.zeros((n, 5), np.uint64)
        self._lib.occluded(self._h, n, _p(o), _p(d), _p(tmax), _p(occ), _p(c))
        return occ, c

    def __del__(self):
        if getattr(self, "_h", None) and getattr(self, "_lib", None) is not None:
            self._lib.scene_free(self._h)
            self._h = None
