"""The test-side restatement of the fork's node-based BSP trees, tests/bspnode_reference.cpp, behind tests/tree_ref.py's
machinery: importing this module registers the restatement's entry points with tree_ref (whose _Lib compiles
tests/<name>_reference.cpp and reads tree_ref._OWN[name]), so that tree_ref itself stays as it is.

    import bspnode_ref
    nodes, idx = bspnode_ref.build(p9, "bspclusterfastkd", n_directions=5, seed=7)
    ref = bspnode_ref.NodeScene(path, "bspcluster", 5, 7)"""
import ctypes as C

import numpy as np

import tree_ref
from tree_ref import _FLT, _INT, _SZ, _U32P, _VP, _p

NAME = "bspnode"
_U32 = C.c_uint32
tree_ref._OWN.setdefault(NAME, ("bspnoderef", {
    "build": (_VP, [_SZ, _VP, _INT, _INT, _INT, _U32, _INT, _INT, _INT, _FLT, _INT, _INT, _U32P]), "copy": (None, [_VP, _VP, _VP]),
    "choose": (_INT, [_INT, _U32, _U32, _SZ, _VP, _U32, _VP, _VP]), "draw_ids": (_INT, [_U32, _U32, _U32, _U32, _VP]),
    "scene_load": (_VP, [C.c_char_p, _INT, _INT, _INT, _U32])}))

CHOOSERS = ("arbitrary", "cluster", "random")
FORMS = ("", "withkd", "fastkd")
ACCELERATORS = tuple("bsp" + c + f for c in CHOOSERS for f in FORMS)
DEFAULT_SEED = 5489
KIND_MASK, LEAF, PLANE = 7, 3, 4      # BSPKdNode's flags (the fastkd trees): 0-2 a kd node's axis, 3 a leaf, 4 a plane node


def split(accelerator):
    """(chooser, form) numbers of an accelerator name"""
    k = ACCELERATORS.index(accelerator)
    return k // 3, k % 3


class NodeScene(tree_ref._TreeScene):
    """A baked scene with the restated node-based tree of (accelerator, K, seed) and default parameters, walked by the restated
    BSP::Intersect / IntersectP, or for a fastkd tree BSPKd::Intersect / IntersectP (a fifth counter: the kd interior nodes)."""
    NAME, NODE_WORDS = NAME, 5

    def __init__(self, path, accelerator, n_directions, seed=DEFAULT_SEED):
        chooser, form = split(accelerator)
        self.COUNTERS = 5 if form == 2 else 4
        self._open(path, chooser, form, n_directions, seed)


def build(p9, accelerator, n_directions=3, seed=DEFAULT_SEED, isect_cost=80, trav_cost=5, kd_trav_cost=1, empty_bonus=0.0, max_prims=1, max_depth=-1):
    """(nodes [n, 5] uint32: the 20-byte BSPNode / BSPKdNode, primitiveIndices) of the restated buildTree over triangles;
    RuntimeError where the reference's build is undefined."""
    p9 = np.ascontiguousarray(p9, np.float32).reshape(-1, 9)
    chooser, form = split(accelerator)
    sizes = (C.c_uint32 * 2)()
    h = tree_ref._load(NAME).build(p9.shape[0], _p(p9), chooser, form, n_directions, seed, isect_cost, trav_cost, kd_trav_cost, empty_bonus, max_prims,
                                   max_depth, sizes)
    return tree_ref._built(NAME, h, sizes, 5)


def choose(chooser, K, seed, p9, draws=1):
    """`draws` calls of calculateDirections over the triangles p9 from one engine: a list of [k, 3] float32 arrays"""
    p9 = np.ascontiguousarray(p9, np.float32).reshape(-1, 9)
    counts = np.zeros(draws, np.uint32); dirs = np.zeros((draws * max(K, p9.shape[0]), 3), np.float32)
    L = tree_ref._load(NAME)
    if L.choose(CHOOSERS.index(chooser), K, seed, p9.shape[0], _p(p9), draws, _p(counts), _p(dirs)):
        raise RuntimeError(L.last_error().decode())
    ends = np.cumsum(counts)
    return [dirs[e - c:e].copy() for c, e in zip(counts, ends)]


def draw_ids(count, np_, seed, draws=1):
    """[draws, count] uint32: the index sets the choosers draw (sorted, as std::set iterates)"""
    ids = np.zeros((draws, count), np.uint32)
    L = tree_ref._load(NAME)
    if L.draw_ids(count, np_, seed, draws, _p(ids)):
        raise RuntimeError(L.last_error().decode())
    return ids


def interior_axes(nodes, fastkd):
    """(is-interior mask, is-axis-aligned mask over all nodes): a fastkd tree's kd nodes, or the BSPNode interiors whose axis is a unit axis"""
    if fastkd:
        kind = nodes[:, 1] & KIND_MASK
        return kind != LEAF, kind < LEAF
    interior = (nodes[:, 1] & 1) == 0
    a = nodes[:, 2:].view(np.float32)
    unit = ((a == 0).sum(1) == 2) & ((a == 1).sum(1) == 1)
    return interior, interior & unit


def assert_same_tree(got, want, fastkd):
    """two (nodes [n, 5], primitiveIndices) are one tree: flags, splits and primitiveIndices everywhere, axes on the nodes that have
    one (the reference leaves the axis words of leaves and of kd nodes uninitialised)"""
    (n0, i0), (n1, i1) = got, want
    assert n0.shape == n1.shape, (n0.shape, n1.shape)
    assert np.array_equal(n0[:, :2], n1[:, :2]), int((n0[:, :2] != n1[:, :2]).any(1).argmax())
    has_axis = ((n1[:, 1] & KIND_MASK) == PLANE) if fastkd else ((n1[:, 1] & 1) == 0)
    assert np.array_equal(n0[has_axis, 2:], n1[has_axis, 2:])
    assert np.array_equal(i0, i1)
