"""ctypes wrappers around the test-side restatements of the fork's tree accelerators, tests/{kd,rbsp,rbspkd,bsppaper}_reference.cpp
over tests/tree_reference.h (build and both walks over the oracle's primitive tests).  Each is compiled with g++ into a
per-process temporary directory on first use — test infrastructure only.  One namespace per accelerator (kd, rbsp, rbspkd,
bsppaper) holds its build function and scene class:  from tree_ref import rbsp as rbsp_ref."""
import ctypes as C
import os
import subprocess
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_libs = {}
_VP, _SZ, _INT, _FLT, _U32P = C.c_void_p, C.c_size_t, C.c_int, C.c_float, C.POINTER(C.c_uint32)
# the entry points the restatements share, <prefix>_<name>: (restype, argtypes); those a restatement lacks are skipped
_SHARED = {
    "last_error": (C.c_char_p, []),
    "free": (None, [_VP]),
    "scene_free": (None, [_VP]),
    "scene_prims": (_SZ, [_VP]),
    "scene_triangles": (_SZ, [_VP, _VP]),
    "scene_tree": (None, [_VP, _U32P, _VP, _VP]),
    "scene_splits": (_SZ, [_VP, _VP, _VP, _SZ]),
    "intersect": (None, [_VP, _SZ, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "occluded": (None, [_VP, _SZ, _VP, _VP, _VP, _VP, _VP]),
    "scene_max_todo": (_SZ, [_VP, _VP]),
    "scene_max_todo_dot": (_SZ, [_VP, _VP]),
}
# and those whose arguments are an accelerator's own
_OWN = {
    "kd": ("kdref", {"build": (_VP, [_SZ, _VP, _VP, _INT, _INT, _FLT, _INT, _INT, _U32P]), "copy": (None, [_VP, _VP, _VP]),
                     "scene_load": (_VP, [C.c_char_p]), "scene_bounds": (None, [_VP, _VP, _VP]),
                     "scene_set_tree": (None, [_VP, _SZ, _VP, _SZ, _VP])}),
    "rbsp": ("rbspref", {"build": (_VP, [_SZ, _VP, _INT, _INT, _INT, _FLT, _INT, _INT, _U32P]), "copy": (None, [_VP, _VP, _VP, _VP]),
                         "scene_load": (_VP, [C.c_char_p, _INT, _INT]), "scene_set_tree": (None, [_VP, _INT, _SZ, _VP, _SZ, _VP])}),
    "rbspkd": ("rbspkdref", {"build": (_VP, [_SZ, _VP, _INT, _INT, _INT, _INT, _FLT, _INT, _INT, _U32P]), "copy": (None, [_VP, _VP, _VP, _VP]),
                             "scene_load": (_VP, [C.c_char_p, _INT, _INT]), "scene_set_tree": (None, [_VP, _INT, _SZ, _VP, _SZ, _VP]),
                             "scene_dot_only": (None, [_VP, _INT])}),
    "bsppaper": ("bspref", {"build": (_VP, [_SZ, _VP, _INT, _INT, _FLT, _INT, _INT, _U32P]), "copy": (None, [_VP, _VP, _VP]),
                            "scene_load": (_VP, [C.c_char_p, _INT]), "scene_set_tree": (None, [_VP, _SZ, _VP, _SZ, _VP]),
                            "planes": (_SZ, [_VP, _VP]), "classify": (None, [_SZ, _VP, _VP, _VP, _VP, _VP, _SZ, _VP])}),
}


class _Lib:
    """tests/<name>_reference.cpp, loaded; its entry points without their prefix"""

    def __init__(self, name):
        prefix, own = _OWN[name]
        out = os.path.join(tempfile.mkdtemp(prefix=prefix), "lib%s.so" % prefix)
        cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function",
               "-I", os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests", name + "_reference.cpp"), "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(name + "_reference.cpp failed to build:\n" + r.stderr)
        L = C.CDLL(out)
        for fn, (restype, argtypes) in list(_SHARED.items()) + list(own.items()):
            f = getattr(L, prefix + "_" + fn, None)
            if f is not None:
                f.restype, f.argtypes = restype, argtypes
                setattr(self, fn, f)


def _load(name):
    if name not in _libs:
        _libs[name] = _Lib(name)
    return _libs[name]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _built(name, h, sizes, node_words, n_directions=None):
    """the arrays of a built tree (and its directions), which is then freed"""
    L = _load(name)
    if not h:
        raise RuntimeError(L.last_error().decode())
    nodes = np.zeros((sizes[0], node_words), np.uint32); idx = np.zeros(max(1, sizes[1]), np.uint32)
    if n_directions is None:
        L.copy(h, _p(nodes), _p(idx))
    else:
        dirs = np.zeros((n_directions, 3), np.float32)
        L.copy(h, _p(nodes), _p(idx), _p(dirs))
    L.free(h)
    return (nodes, idx[:sizes[1]]) + (() if n_directions is None else (dirs,))


class _TreeScene:
    """A baked scene with a tree of `NAME`'s restatement: nodes of NODE_WORDS words, COUNTERS counter columns per ray."""
    NAME, NODE_WORDS, COUNTERS = None, 2, 4

    def _open(self, path, *args):
        self._lib = _load(self.NAME)
        self._h = self._lib.scene_load(path.encode(), *args)
        if not self._h:
            raise RuntimeError(self._lib.last_error().decode())
        self.n = self._lib.scene_prims(self._h)

    def _set_tree(self, nodes, idx, *args):
        nodes = np.ascontiguousarray(nodes, np.uint32); idx = np.ascontiguousarray(idx, np.uint32)
        self._lib.scene_set_tree(self._h, *args, nodes.shape[0], _p(nodes), idx.shape[0], _p(idx))

    def triangles(self):
        """[k, 9] float32: the scene's triangles in creation order (other primitives skipped)"""
        p9 = np.zeros((self.n, 9), np.float32)
        k = self._lib.scene_triangles(self._h, _p(p9))
        return p9[:k]

    def tree(self):
        sizes = (C.c_uint32 * 2)()
        self._lib.scene_tree(self._h, sizes, None, None)
        nodes = np.zeros((sizes[0], self.NODE_WORDS), np.uint32); idx = np.zeros(max(1, sizes[1]), np.uint32)
        self._lib.scene_tree(self._h, sizes, _p(nodes), _p(idx))
        return nodes, idx[:sizes[1]]

    def splits(self, cap=4096):
        ax = np.zeros(cap, np.int32); pos = np.zeros(cap, np.float32)
        k = self._lib.scene_splits(self._h, _p(ax), _p(pos), cap)
        return ax[:k], pos[:k]

    def intersect(self, o, d, tmax):
        """t, primitive, barycentrics and per ray the counters nodes, interior nodes, triangle tests, sphere tests (rbspkd: and
        the kd interior nodes)"""
        o = np.ascontiguousarray(o, np.float32); d = np.ascontiguousarray(d, np.float32); tmax = np.ascontiguousarray(tmax, np.float32)
        n = tmax.shape[0]
        t = np.zeros(n, np.float32); prim = np.zeros(n, np.int32); bary = np.zeros((n, 3), np.float32); c = np.zeros((n, self.COUNTERS), np.uint64)
        self._lib.intersect(self._h, n, _p(o), _p(d), _p(tmax), _p(t), _p(prim), _p(bary), _p(c))
        return t, prim, bary, c

    def occluded(self, o, d, tmax):
        o = np.ascontiguousarray(o, np.float32); d = np.ascontiguousarray(d, np.float32); tmax = np.ascontiguousarray(tmax, np.float32)
        n = tmax.shape[0]
        occ = np.zeros(n, np.uint8); c = np.zeros((n, self.COUNTERS), np.uint64)
        self._lib.occluded(self._h, n, _p(o), _p(d), _p(tmax), _p(occ), _p(c))
        return occ, c

    def max_todo(self):
        """per ray of the last intersect() / occluded() call, the largest todoPos the walk reached: the todo entries it held at once"""
        n = self._lib.scene_max_todo(self._h, None)
        out = np.zeros(n, np.uint32)
        self._lib.scene_max_todo(self._h, _p(out))
        return out

    def max_todo_dot(self):
        """as max_todo, over the pushes made at interior nodes the walk does not take as kd nodes (rbspkd: the dot-product step)"""
        n = self._lib.scene_max_todo_dot(self._h, None)
        out = np.zeros(n, np.uint32)
        self._lib.scene_max_todo_dot(self._h, _p(out))
        return out

    def __del__(self):
        # the library hangs off the instance: module globals are cleared at interpreter exit
        if getattr(self, "_h", None) and getattr(self, "_lib", None) is not None:
            self._lib.scene_free(self._h)
            self._h = None


class KdScene(_TreeScene):
    """A baked scene with the default kd-tree (intersectcost 80, traversalcost 1, emptybonus 0, maxprims 1, maxdepth -1), or a
    tree given by set_tree()."""
    NAME = "kd"

    def __init__(self, path):
        self._open(path)

    def set_tree(self, nodes, idx):
        self._set_tree(nodes, idx)

    def bounds(self):
        lo = np.zeros((self.n, 3), np.float32); hi = np.zeros((self.n, 3), np.float32)
        self._lib.scene_bounds(self._h, _p(lo), _p(hi))
        return lo, hi


class RbspScene(_TreeScene):
    """A baked scene with an RBSP tree: the restated default build (build=True), or a tree given by set_tree()."""
    NAME = "rbsp"

    def __init__(self, path, n_directions=3, build=True):
        self.M = n_directions
        self._open(path, n_directions, 1 if build else 0)

    def set_tree(self, nodes, idx):
        self._set_tree(nodes, idx, self.M)


class RbspKdScene(RbspScene):
    """A baked scene with an rbspkd tree: the restated default build (build=True), or a tree given by set_tree().  dot_only(True)
    walks every interior node with RBSP's dot-product step instead (the control).  The fifth counter is the kd interior nodes."""
    NAME, COUNTERS = "rbspkd", 5

    def dot_only(self, on):
        self._lib.scene_dot_only(self._h, 1 if on else 0)


class BspScene(_TreeScene):
    """A baked scene with a general BSP tree: the restated default build (build=True), or a tree given by set_tree()."""
    NAME, NODE_WORDS = "bsppaper", 5

    def __init__(self, path, build=True):
        self._open(path, 1 if build else 0)

    def set_tree(self, nodes, idx):
        self._set_tree(nodes, idx)


def _kd_build(bmin, bmax, isect_cost=80, trav_cost=1, empty_bonus=0.0, max_prims=1, max_depth=-1):
    """(nodes [n, 2] uint32, primitiveIndices) of the restated KdTreeAccel::buildTree."""
    bmin = np.ascontiguousarray(bmin, np.float32); bmax = np.ascontiguousarray(bmax, np.float32)
    sizes = (C.c_uint32 * 2)()
    h = _load("kd").build(bmin.shape[0], _p(bmin), _p(bmax), isect_cost, trav_cost, empty_bonus, max_prims, max_depth, sizes)
    return _built("kd", h, sizes, 2)


def _rbsp_build(p9, n_directions=3, isect_cost=80, trav_cost=5, empty_bonus=0.0, max_prims=1, max_depth=-1):
    """(nodes [n, 2] uint32, primitiveIndices, directions [M, 3]) of the restated RBSP::buildTree over triangles."""
    p9 = np.ascontiguousarray(p9, np.float32).reshape(-1, 9)
    sizes = (C.c_uint32 * 2)()
    h = _load("rbsp").build(p9.shape[0], _p(p9), n_directions, isect_cost, trav_cost, empty_bonus, max_prims, max_depth, sizes)
    return _built("rbsp", h, sizes, 2, n_directions)


def _rbspkd_build(p9, n_directions=3, isect_cost=80, trav_cost=5, kd_trav_cost=1, empty_bonus=0.0, max_prims=1, max_depth=-1):
    """(nodes [n, 2] uint32, primitiveIndices, directions [M, 3]) of the restated RBSPKd::buildTree over triangles; RuntimeError
    where the reference's build is undefined."""
    p9 = np.ascontiguousarray(p9, np.float32).reshape(-1, 9)
    sizes = (C.c_uint32 * 2)()
    h = _load("rbspkd").build(p9.shape[0], _p(p9), n_directions, isect_cost, trav_cost, kd_trav_cost, empty_bonus, max_prims, max_depth, sizes)
    return _built("rbspkd", h, sizes, 2, n_directions)


def _bsp_build(p9, isect_cost=80, trav_cost=5, empty_bonus=0.0, max_prims=1, max_depth=-1):
    """(nodes [n, 5] uint32: the 20-byte BSPNode, primitiveIndices) of the restated BSPPaper::buildTree over triangles."""
    p9 = np.ascontiguousarray(p9, np.float32).reshape(-1, 9)
    sizes = (C.c_uint32 * 2)()
    h = _load("bsppaper").build(p9.shape[0], _p(p9), isect_cost, trav_cost, empty_bonus, max_prims, max_depth, sizes)
    return _built("bsppaper", h, sizes, 5)


def _bsp_planes(tri9):
    """[k, 4] float32 {t, axis} of Triangle::getBSPPaperPlanes"""
    tri9 = np.ascontiguousarray(tri9, np.float32).reshape(9)
    out = np.zeros((4, 4), np.float32)
    k = _load("bsppaper").planes(_p(tri9), _p(out))
    return out[:k]


def _bsp_classify(p9, plane4):
    """((left, right) counts of getAmountToLeftAndRight, left list, right list of getPrimnumsToLeftAndRight)"""
    p9 = np.ascontiguousarray(p9, np.float32).reshape(-1, 9); plane4 = np.ascontiguousarray(plane4, np.float32)
    n = p9.shape[0]
    counts = np.zeros(2, np.uint32); left = np.zeros(2 * n + 1, np.uint32); right = np.zeros(2 * n + 1, np.uint32); sizes = np.zeros(2, np.uint32)
    _load("bsppaper").classify(n, _p(p9), _p(plane4), _p(counts), _p(left), _p(right), 2 * n + 1, _p(sizes))
    return tuple(int(c) for c in counts), left[:sizes[0]], right[:sizes[1]]


kd = types.SimpleNamespace(build=_kd_build, KdScene=KdScene)
rbsp = types.SimpleNamespace(build=_rbsp_build, RbspScene=RbspScene)
rbspkd = types.SimpleNamespace(build=_rbspkd_build, RbspKdScene=RbspKdScene)
bsppaper = types.SimpleNamespace(build=_bsp_build, planes=_bsp_planes, classify=_bsp_classify, BspScene=BspScene)
