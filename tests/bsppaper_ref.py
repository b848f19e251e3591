"""ctypes wrapper around tests/bsppaper_reference.cpp, the test-side restatement of the fork's general BSP tree (build, the BVH
classifications, the planes of a triangle and both walks over the oracle's primitive tests).  Compiled with g++ into a per-process
temporary directory on first use — test infrastructure only."""
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
        out = os.path.join(tempfile.mkdtemp(prefix="bspref"), "libbspref.so")
        cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function",
               "-I", os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests", "bsppaper_reference.cpp"), "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("bsppaper_reference.cpp failed to build:\n" + r.stderr)
        L = C.CDLL(out)
        vp, sz, u32p = C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)
        L.bspref_last_error.restype = C.c_char_p
        L.bspref_build.restype = vp
        L.bspref_build.argtypes = [sz, vp, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, u32p]
        L.bspref_copy.argtypes = [vp, vp, vp]
        L.bspref_free.argtypes = [vp]
        L.bspref_planes.restype = sz
        L.bspref_planes.argtypes = [vp, vp]
        L.bspref_classify.argtypes = [sz, vp, vp, vp, vp, vp, sz, vp]
        L.bspref_scene_load.restype = vp
        L.bspref_scene_load.argtypes = [C.c_char_p, C.c_int]
        L.bspref_scene_set_tree.argtypes = [vp, sz, vp, sz, vp]
        L.bspref_scene_free.argtypes = [vp]
        L.bspref_scene_prims.restype = sz
        L.bspref_scene_prims.argtypes = [vp]
        L.bspref_scene_triangles.restype = sz
        L.bspref_scene_triangles.argtypes = [vp, vp]
        L.bspref_scene_tree.argtypes = [vp, u32p, vp, vp]
        L.bspref_intersect.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, vp]
        L.bspref_occluded.argtypes = [vp, sz, vp, vp, vp, vp, vp]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def build(p9, isect_cost=80, trav_cost=5, empty_bonus=0.0, max_prims=1, max_depth=-1):
    """(nodes [n, 5] uint32: the 20-byte BSPNode, primitiveIndices) of the restated BSPPaper::buildTree over triangles."""
    p9 = np.ascontiguousarray(p9, np.float32).reshape(-1, 9)
    sizes = (C.c_uint32 * 2)()
    h = lib().bspref_build(p9.shape[0], _p(p9), isect_cost, trav_cost, empty_bonus, max_prims, max_depth, sizes)
    nodes = np.zeros((sizes[0], 5), np.uint32); idx = np.zeros(max(1, sizes[1]), np.uint32)
    lib().bspref_copy(h, _p(nodes), _p(idx))
    lib().bspref_free(h)
    return nodes, idx[:sizes[1]]


def planes(tri9):
    """[k, 4] float32 {t, axis} of Triangle::getBSPPaperPlanes"""
    tri9 = np.ascontiguousarray(tri9, np.float32).reshape(9)
    out = np.zeros((4, 4), np.float32)
    k = lib().bspref_planes(_p(tri9), _p(out))
    return out[:k]


def classify(p9, plane4):
    """((left, right) counts of getAmountToLeftAndRight, left list, right list of getPrimnumsToLeftAndRight)"""
    p9 = np.ascontiguousarray(p9, np.float32).reshape(-1, 9); plane4 = np.ascontiguousarray(plane4, np.float32)
    n = p9.shape[0]
    counts = np.zeros(2, np.uint32); left = np.zeros(2 * n + 1, np.uint32); right = np.zeros(2 * n + 1, np.uint32); sizes = np.zeros(2, np.uint32)
    lib().bspref_classify(n, _p(p9), _p(plane4), _p(counts), _p(left), _p(right), 2 * n + 1, _p(sizes))
    return tuple(int(c) for c in counts), left[:sizes[0]], right[:sizes[1]]


class BspScene:
    """A baked scene with a general BSP tree: the restated default build (build=True), or a tree given by set_tree()."""

    def __init__(self, path, build=True):
        self._h = lib().bspref_scene_load(path.encode(), 1 if build else 0)
        if not self._h:
            raise RuntimeError(lib().bspref_last_error().decode())
        self.n = lib().bspref_scene_prims(self._h)

    def set_tree(self, nodes, idx):
        nodes = np.ascontiguousarray(nodes, np.uint32); idx = np.ascontiguousarray(idx, np.uint32)
        lib().bspref_scene_set_tree(self._h, nodes.shape[0], _p(nodes), idx.shape[0], _p(idx))

    def triangles(self):
        """[k, 9] float32: the scene's triangles in creation order (other primitives skipped)"""
        p9 = np.zeros((self.n, 9), np.float32)
        k = lib().bspref_scene_triangles(self._h, _p(p9))
        return p9[:k]

    def tree(self):
        sizes = (C.c_uint32 * 2)()
        lib().bspref_scene_tree(self._h, sizes, None, None)
        nodes = np.zeros((sizes[0], 5), np.uint32); idx = np.zeros(max(1, sizes[1]), np.uint32)
        lib().bspref_scene_tree(self._h, sizes, _p(nodes), _p(idx))
        return nodes, idx[:sizes[1]]

    def intersect(self, o, d, tmax):
        o = np.ascontiguousarray(o, np.float32); d = np.ascontiguousarray(d, np.float32); tmax = np.ascontiguousarray(tmax, np.float32)
        n = tmax.shape[0]
        t = np.zeros(n, np.float32); prim = np.zeros(n, np.int32); bary = np.zeros((n, 3), np.float32); c = np.zeros((n, 4), np.uint64)
        lib().bspref_intersect(self._h, n, _p(o), _p(d), _p(tmax), _p(t), _p(prim), _p(bary), _p(c))
        return t, prim, bary, c

    def occluded(self, o, d, tmax):
        o = np.ascontiguousarray(o, np.float32); d = np.ascontiguousarray(d, np.float32); tmax = np.ascontiguousarray(tmax, np.float32)
        n = tmax.shape[0]
        occ = np.zeros(n, np.uint8); c = np.zeros((n, 4), np.uint64)
        lib().bspref_occluded(self._h, n, _p(o), _p(d), _p(tmax), _p(occ), _p(c))
        return occ, c

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:      # (module globals are cleared at interpreter exit)
            _lib.bspref_scene_free(self._h)
            self._h = None
