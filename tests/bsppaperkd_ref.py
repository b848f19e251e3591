"""The test-side restatement of the fork's kd-aware general BSP tree, tests/bsppaperkd_reference.cpp, behind tests/tree_ref.py's
machinery: importing this module registers the restatement's entry points with tree_ref (whose _Lib compiles
tests/<name>_reference.cpp and reads tree_ref._OWN[name]), so that tree_ref itself stays as it is.

    import bsppaperkd_ref
    nodes, idx = bsppaperkd_ref.build(p9, kd_trav_cost=5)
    ref = bsppaperkd_ref.BspKdScene(path)"""
import ctypes as C

import numpy as np

import tree_ref
from tree_ref import _FLT, _INT, _SZ, _U32P, _VP, _p

NAME = "bsppaperkd"
tree_ref._OWN.setdefault(NAME, ("bspkdref", {"build": (_VP, [_SZ, _VP, _INT, _INT, _INT, _FLT, _INT, _INT, _U32P]), "copy": (None, [_VP, _VP, _VP]),
                                             "scene_load": (_VP, [C.c_char_p, _INT]), "scene_set_tree": (None, [_VP, _SZ, _VP, _SZ, _VP]),
                                             "scene_dot_only": (None, [_VP, _INT])}))

KIND_MASK, LEAF, PLANE, SHIFT = 7, 3, 4, 3      # BSPKdNode's flags: 0-2 a kd node's axis, 3 a leaf, 4 a plane node


class BspKdScene(tree_ref._TreeScene):
    """A baked scene with a bsppaperkd tree: the restated default build (build=True), or a tree given by set_tree().
    dot_only(True) walks every interior node with the dot-product step instead (the control).  The fifth counter is the kd
    interior nodes."""
    NAME, NODE_WORDS, COUNTERS = NAME, 5, 5

    def __init__(self, path, build=True):
        self._open(path, 1 if build else 0)

    def set_tree(self, nodes, idx):
        self._set_tree(nodes, idx)

    def dot_only(self, on):
        self._lib.scene_dot_only(self._h, 1 if on else 0)


def build(p9, isect_cost=80, trav_cost=5, kd_trav_cost=1, empty_bonus=0.0, max_prims=1, max_depth=-1):
    """(nodes [n, 5] uint32: the 20-byte BSPKdNode, primitiveIndices) of the restated BSPPaperKd::buildTree over triangles."""
    p9 = np.ascontiguousarray(p9, np.float32).reshape(-1, 9)
    sizes = (C.c_uint32 * 2)()
    h = tree_ref._load(NAME).build(p9.shape[0], _p(p9), isect_cost, trav_cost, kd_trav_cost, empty_bonus, max_prims, max_depth, sizes)
    return tree_ref._built(NAME, h, sizes, 5)


def kinds(nodes):
    """the node kinds (flags & 7) and the counts of kd, plane and leaf nodes"""
    k = nodes[:, 1] & KIND_MASK
    return k, int((k < LEAF).sum()), int((k == PLANE).sum()), int((k == LEAF).sum())


def assert_same_tree(got, want):
    """two (nodes [n, 5], primitiveIndices) are one tree: flags, splits and primitiveIndices everywhere, axes on plane nodes only (the
    reference leaves the axis words of kd nodes and leaves uninitialised)"""
    (n0, i0), (n1, i1) = got, want
    assert n0.shape == n1.shape, (n0.shape, n1.shape)
    assert np.array_equal(n0[:, :2], n1[:, :2]), int((n0[:, :2] != n1[:, :2]).any(1).argmax())
    plane = (n1[:, 1] & KIND_MASK) == PLANE
    assert np.array_equal(n0[plane, 2:], n1[plane, 2:])
    assert np.array_equal(i0, i1)
