"""ctypes wrapper around tests/rbsp_reference.cpp, the test-side restatement of the fork's RBSP tree (build and both walks over
the oracle's primitive tests).  Compiled with g++ into a per-process temporary directory on first use — test infrastructure only."""
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
        out = os.path.join(tempfile.mkdtemp(prefix="rbspref"), "librbspref.so")
        cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function",
               "-I", os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests", "rbsp_reference.cpp"), "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("rbsp_reference.cpp failed to build:\n" + r.stderr)
        L = C.CDLL(out)
        vp, sz, u32p = C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)
        L.rbspref_last_error.restype = C.c_char_p
        L.rbspref_build.restype = vp
        L.rbspref_build.argtypes = [sz, vp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, u32p]
        L.rbspref_copy.argtypes = [vp, vp, vp, vp]
        L.rbspref_free.argtypes = [vp]
        L.rbspref_scene_load.restype = vp
        L.rbspref_scene_load.argtypes = [C.c_char_p, C.c_int, C.c_int]
        L.rbspref_scene_set_tree.argtypes = [vp, C.c_int, sz, vp, sz, vp]
        L.rbspref_scene_free.argtypes = [vp]
        L.rbspref_scene_prims.restype = sz
        L.rbspref_scene_prims.argtypes = [vp]
        L.rbspref_scene_triangles.restype = sz
        L.rbspref_scene_triangles.argtypes = [vp, vp]
        L.rbspref_scene_tree.argtypes = [vp, u32p, vp, vp]
        L.rbspref_scene_splits.restype = sz
        L.rbspref_scene_splits.argtypes = [vp, vp, vp, sz]
        L.rbspref_intersect.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, vp]
        L.rbspref_occluded.argtypes = [vp, sz, vp, vp, vp, vp, vp]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def build(p9, n_directions=3, isect_cost=80, trav_cost=5, empty_bonus=0.0, max_prims=1, max_depth=-1):
    """(nodes [n, 2] uint32, primitiveIndices, directions [M, 3]) of the restated RBSP::buildTree over triangles."""
    p9 = np.ascontiguousarray(p9, np.float32).reshape(-1, 9)
    sizes = (C.c_uint32 * 2)()
    h = lib().rbspref_build(p9.shape[0], _p(p9), n_directions, isect_cost, trav_cost, empty_bonus, max_prims, max_depth, sizes)
    nodes = np.zeros((sizes[0], 2), np.uint32); idx = np.zeros(max(1, sizes[1]), np.uint32); dirs = np.zeros((n_directions, 3), np.float32)
    lib().rbspref_copy(h, _p(nodes), _p(idx), _p(dirs))
    lib().rbspref_free(h)
    return nodes, idx[:sizes[1]], dirs


class RbspScene:
    """A baked scene with an RBSP tree: the restated default build (build=True), or a tree given by set_tree()."""

    def __init__(self, path, n_directions=3, build=True):
        self.M = n_directions
        self._h = lib().rbspref_scene_load(path.encode(), n_directions, 1 if build else 0)
        if not self._h:
            raise RuntimeError(lib().rbspref_last_error().decode())
        self.n = lib().rbspref_scene_prims(self._h)

    def set_tree(self, nodes, idx):
        nodes = np.ascontiguousarray(nodes, np.uint32); idx = np.ascontiguousarray(idx, np.uint32)
        lib().rbspref_scene_set_tree(self._h, self.M, nodes.shape[0], _p(nodes), idx.shape[0], _p(idx))

    def triangles(self):
        """[k, 9] float32: the scene's triangles in creation order (other primitives skipped)"""
        p9 = np.zeros((self.n, 9), np.float32)
        k = lib().rbspref_scene_triangles(self._h, _p(p9))
        return p9[:k]

    def tree(self):
        sizes = (C.c_uint32 * 2)()
        lib().rbspref_scene_tree(self._h, sizes, None, None)
        nodes = np.zeros((sizes[0], 2), np.uint32); idx = np.zeros(max(1, sizes[1]), np.uint32)
        lib().rbspref_scene_tree(self._h, sizes, _p(nodes), _p(idx))
        return nodes, idx[:sizes[1]]

    def splits(self, cap=4096):
        ax = np.zeros(cap, np.int32); pos = np.zeros(cap, np.float32)
        k = lib().rbspref_scene_splits(self._h, _p(ax), _p(pos), cap)
        return ax[:k], pos[:k]

    def intersect(self, o, d, tmax):
        o = np.ascontiguousarray(o, np.float32); d = np.ascontiguousarray(d, np.float32); tmax = np.ascontiguousarray(tmax, np.float32)
        n = tmax.shape[0]
        t = np.zeros(n, np.float32); prim = np.zeros(n, np.int32); bary = np.zeros((n, 3), np.float32); c = np.zeros((n, 4), np.uint64)
        lib().rbspref_intersect(self._h, n, _p(o), _p(d), _p(tmax), _p(t), _p(prim), _p(bary), _p(c))
        return t, prim, bary, c

    def occluded(self, o, d, tmax):
        o = np.ascontiguousarray(o, np.float32); d = np.ascontiguousarray(d, np.float32); tmax = np.ascontiguousarray(tmax, np.float32)
        n = tmax.shape[0]
        occ = np.zeros(n, np.uint8); c = np.zeros((n, 4), np.uint64)
        lib().rbspref_occluded(self._h, n, _p(o), _p(d), _p(tmax), _p(occ), _p(c))
        return occ, c

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:      # (module globals are cleared at interpreter exit)
            _lib.rbspref_scene_free(self._h)
            self._h = None
