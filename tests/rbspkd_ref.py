"""ctypes wrapper around tests/rbspkd_reference.cpp, the test-side restatement of the fork's kd-aware RBSP tree (RBSPKd: build
and both walks over the oracle's primitive tests, with the kd / bsp split of the interior-node counts).  Compiled with g++ into a per-process temporary directory on first use — test infrastructure only."""
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
        out = os.path.join(tempfile.mkdtemp(prefix="rbspkdref"), "librbspkdref.so")
        cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function",
               "-I", os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests", "rbspkd_reference.cpp"), "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("rbspkd_reference.cpp failed to build:\n" + r.stderr)
        L = C.CDLL(out)
        vp, sz, u32p = C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)
        L.rbspkdref_last_error.restype = C.c_char_p
        L.rbspkdref_build.restype = vp
        L.rbspkdref_build.argtypes = [sz, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, u32p]
        L.rbspkdref_scene_dot_only.argtypes = [vp, C.c_int]
        L.rbspkdref_copy.argtypes = [vp, vp, vp, vp]
        L.rbspkdref_free.argtypes = [vp]
        L.rbspkdref_scene_load.restype = vp
        L.rbspkdref_scene_load.argtypes = [C.c_char_p, C.c_int, C.c_int]
        L.rbspkdref_scene_set_tree.argtypes = [vp, C.c_int, sz, vp, sz, vp]
        L.rbspkdref_scene_free.argtypes = [vp]
        L.rbspkdref_scene_prims.restype = sz
        L.rbspkdref_scene_prims.argtypes = [vp]
        L.rbspkdref_scene_triangles.restype = sz
        L.rbspkdref_scene_triangles.argtypes = [vp, vp]
        L.rbspkdref_scene_tree.argtypes = [vp, u32p, vp, vp]
        L.rbspkdref_scene_splits.restype = sz
        L.rbspkdref_scene_splits.argtypes = [vp, vp, vp, sz]
        L.rbspkdref_intersect.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, vp]
        L.rbspkdref_occluded.argtypes = [vp, sz, vp, vp, vp, vp, vp]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def build(p9, n_directions=3, isect_cost=80, trav_cost=5, kd_trav_cost=1, empty_bonus=0.0, max_prims=1, max_depth=-1):
    """(nodes [n, 2] uint32, primitiveIndices, directions [M, 3]) of the restated RBSPKd::buildTree over triangles."""
    p9 = np.ascontiguousarray(p9, np.float32).reshape(-1, 9)
    sizes = (C.c_uint32 * 2)()
    h = lib().rbspkdref_build(p9.shape[0], _p(p9), n_directions, isect_cost, trav_cost, kd_trav_cost, empty_bonus, max_prims, max_depth, sizes)
    if not h:
        raise RuntimeError(lib().rbspkdref_last_error().decode())
    nodes = np.zeros((sizes[0], 2), np.uint32); idx = np.zeros(max(1, sizes[1]), np.uint32); dirs = np.zeros((n_directions, 3), np.float32)
    lib().rbspkdref_copy(h, _p(nodes), _p(idx), _p(dirs))
    lib().rbspkdref_free(h)
    return nodes, idx[:sizes[1]], dirs


class RbspKdScene:
    """A baked scene with an rbspkd tree: the restated default build (build=True), or a tree given by set_tree().  dot_only(True)
    walks every interior node with RBSP's dot-product step instead (the control)."""

    def __init__(self, path, n_directions=3, build=True):
        self.M = n_directions
        self._h = lib().rbspkdref_scene_load(path.encode(), n_directions, 1 if build else 0)
        if not self._h:
            raise RuntimeError(lib().rbspkdref_last_error().decode())
        self.n = lib().rbspkdref_scene_prims(self._h)

    def dot_only(self, on):
        lib().rbspkdref_scene_dot_only(self._h, 1 if on else 0)

    def set_tree(self, nodes, idx):
        nodes = np.ascontiguousarray(nodes, np.uint32); idx = np.ascontiguousarray(idx, np.uint32)
        lib().rbspkdref_scene_set_tree(self._h, self.M, nodes.shape[0], _p(nodes), idx.shape[0], _p(idx))

    def triangles(self):
        """[k, 9] float32: the scene's triangles in creation order (other primitives skipped)"""
        p9 = np.zeros((self.n, 9), np.float32)
        k = lib().rbspkdref_scene_triangles(self._h, _p(p9))
        return p9[:k]

    def tree(self):
        sizes = (C.c_uint32 * 2)()
        lib().rbspkdref_scene_tree(self._h, sizes, None, None)
        nodes = np.zeros((sizes[0], 2), np.uint32); idx = np.zeros(max(1, sizes[1]), np.uint32)
        lib().rbspkdref_scene_tree(self._h, sizes, _p(nodes), _p(idx))
        return nodes, idx[:sizes[1]]

    def splits(self, cap=4096):
        ax = np.zeros(cap, np.int32); pos = np.zeros(cap, np.float32)
        k = lib().rbspkdref_scene_splits(self._h, _p(ax), _p(pos), cap)
        return ax[:k], pos[:k]

    def intersect(self, o, d, tmax):
        o = np.ascontiguousarray(o, np.float32); d = np.ascontiguousarray(d, np.float32); tmax = np.ascontiguousarray(tmax, np.float32)
        n = tmax.shape[0]
        t = np.zeros(n, np.float32); prim = np.zeros(n, np.int32); bary = np.zeros((n, 3), np.float32); c = np.zeros((n, 5), np.uint64)
        lib().rbspkdref_intersect(self._h, n, _p(o), _p(d), _p(tmax), _p(t), _p(prim), _p(bary), _p(c))
        return t, prim, bary, c          # c: nodes, interior (kd + bsp), triangle tests, sphere tests, kd interior

    def occluded(self, o, d, tmax):
        o = np.ascontiguousarray(o, np.float32); d = np.ascontiguousarray(d, np.float32); tmax = np.ascontiguousarray(tmax, np.float32)
        n = tmax.shape[0]
        occ = np.zeros(n, np.uint8); c = np.zeros((n, 5), np.uint64)
        lib().rbspkdref_occluded(self._h, n, _p(o), _p(d), _p(tmax), _p(occ), _p(c))
        return occ, c

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:      # (module globals are cleared at interpreter exit)
            _lib.rbspkdref_scene_free(self._h)
            self._h = None
