"""ctypes wrapper around tests/bspnodeinst_reference.cpp, the test-side restatement of the two-level BUILD of an instanced scene
under a node-based accelerator: the oracle's loader gives the primitive lists (an instance is a primitive with a zero normal and
its world bound), tests/bspnode_reference.cpp's BuildNodeBased / BuildFastKd build over them, every tree from a fresh
std::mt19937(seed).  Compiled with g++ into a per-process temporary directory on first use — test infrastructure only.  The
restated two-level WALK is tests/bsppaperinst_ref.py's BspPaperInstScene.take(handle): it walks any trees of this node layout."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import bspnode_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCELERATORS = bspnode_ref.ACCELERATORS
_lib = None
_VP, _SZ, _INT, _U32 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32
_SIG = {
    "last_error": (C.c_char_p, []),
    "scene_load": (_VP, [C.c_char_p]),
    "scene_free": (None, [_VP]),
    "counts": (None, [_VP, _VP]),
    "prims": (_SZ, [_VP, _INT, _VP, _VP, _VP, _VP]),
    "build": (_VP, [_VP, _INT, _INT, _INT, _INT, _U32, _INT, _INT, _INT, C.c_float, _INT, _INT, _VP]),
    "built_copy": (None, [_VP, _VP, _VP, _VP]),
    "built_free": (None, [_VP]),
}


def _load():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="bspnodeinstref"), "libbspnodeinstref.so")
        cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function",
               "-I", os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests", "bspnodeinst_reference.cpp"), "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("bspnodeinst_reference.cpp failed to build:\n" + r.stderr)
        L = C.CDLL(out)
        for name, (restype, argtypes) in _SIG.items():
            f = getattr(L, "bspnodeinstref_" + name)
            f.restype, f.argtypes = restype, argtypes
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def fastkd(accelerator):
    return accelerator.endswith("fastkd")


class BspNodeInstBuild:
    """A baked scene with object instances: the primitive lists its trees are built over, and the restated builds."""

    def __init__(self, path):
        self._lib = _load()
        self._h = self._lib.bspnodeinstref_scene_load(path.encode())
        if not self._h:
            raise RuntimeError(self._lib.bspnodeinstref_last_error().decode())
        c = np.zeros(3, np.uint32)
        self._lib.bspnodeinstref_counts(self._h, _p(c))
        self.n_top, self.n_objects, self.n_instances = (int(v) for v in c)

    def prims(self, obj=-1):
        """(is_tri [n] uint8, p9 [n, 9], bmin [n, 3], bmax [n, 3]) of the top level (obj < 0) or of one object, in creation order"""
        n = self._lib.bspnodeinstref_prims(self._h, obj, None, None, None, None)
        tri = np.zeros(n, np.uint8); p9 = np.zeros((n, 9), np.float32); lo = np.zeros((n, 3), np.float32); hi = np.zeros((n, 3), np.float32)
        self._lib.bspnodeinstref_prims(self._h, obj, _p(tri), _p(p9), _p(lo), _p(hi))
        return tri, p9, lo, hi

    def build(self, obj, accelerator, n_directions=3, seed=bspnode_ref.DEFAULT_SEED, isect_cost=80, trav_cost=5, kd_trav_cost=1, empty_bonus=0.0,
              max_prims=1, max_depth=-1):
        """(nodes [n, 5] uint32, prim_indices, bounds [6]) of the restated build over prims(obj); RuntimeError where the reference's
        build is undefined"""
        chooser, form = bspnode_ref.split(accelerator)
        sizes = np.zeros(2, np.uint32)
        t = self._lib.bspnodeinstref_build(self._h, obj, chooser, form, n_directions, seed, isect_cost, trav_cost, kd_trav_cost, empty_bonus, max_prims,
                                           max_depth, _p(sizes))
        if not t:
            raise RuntimeError(self._lib.bspnodeinstref_last_error().decode())
        nodes = np.zeros((int(sizes[0]), 5), np.uint32); idx = np.zeros(int(sizes[1]), np.uint32); b = np.zeros(6, np.float32)
        self._lib.bspnodeinstref_built_copy(t, _p(nodes), _p(idx), _p(b))
        self._lib.bspnodeinstref_built_free(t)
        return nodes, idx, b

    def tree_objects(self):
        """the object definitions that get a tree (more than one primitive, core/api.cpp:1798)"""
        return [o for o in range(self.n_objects) if self._lib.bspnodeinstref_prims(self._h, o, None, None, None, None) > 1]

    def __del__(self):
        if getattr(self, "_h", None) and getattr(self, "_lib", None) is not None:
            self._lib.bspnodeinstref_scene_free(self._h)
            self._h = None


def assert_same_trees(handle, ref, accelerator, **kw):
    """every tree of an hprt.BspNodeInst equals the restated build byte for byte: nodes, axes, primitiveIndices, and the bounds"""
    for obj in [-1] + ref.tree_objects():
        wn, wi, wb = ref.build(obj, accelerator, **kw)
        nodes, idx = handle.copy() if obj < 0 else handle.object_copy(obj)
        assert nodes.shape == wn.shape, (accelerator, kw, obj, nodes.shape, wn.shape)
        assert nodes.tobytes() == wn.tobytes() and idx.tobytes() == wi.tobytes(), (accelerator, kw, obj)
        assert handle.bounds(obj).tobytes() == wb.tobytes(), (accelerator, kw, obj)
