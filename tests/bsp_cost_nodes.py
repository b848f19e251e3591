"""Shared by tests/test_bsp_cost_host.py and tests/test_gpu_bsp_cost.py: the inputs of the general BSP candidate-costing tests and
thin wrappers over the two diagnostics hooks.  The nodes come from the builder itself (hprt_debug_bsp_root_nodes hands out the
first nodes of a real build: mesh, directions, candidates, the BVH over the node's primitives and the build's primitives, with the
costs and counts the builder's own code gave them); hprt_debug_bsp_cost costs them again with impl 0 (the vector code plus
NodeBvh::count), 1 (bsp_cost.h on the host) or 2 (k_bspcost).  The soups are those of tests/kdop_cost_nodes.py."""
import ctypes as C
import functools
import os

import numpy as np

from conftest import GOLDEN
from kdop_cost_nodes import soups, same_bits      # noqa: F401  (same_bits is re-exported)

DODECA = os.path.join(GOLDEN, "dodecahedron.hprt")
EDGE = np.dtype([("v1", np.float32, 3), ("v2", np.float32, 3), ("f1", np.uint32), ("f2", np.uint32)])
CAND = np.dtype([("k", np.uint32), ("i", np.uint32), ("nBelow", np.uint32), ("nAbove", np.uint32), ("t", np.float32), ("axis", np.float32, 3)])
SCALARS = np.dtype([("invTotalSA", np.float32), ("emptyBonus", np.float32), ("isectCost", np.uint32), ("traversalCost", np.uint32),
                    ("kdTraversalCost", np.uint32), ("nPrimitives", np.uint32), ("maxEdges", np.uint32), ("maxFaces", np.uint32),
                    ("maxFaceEdges", np.uint32), ("maxStack", np.uint32)])
BVHNODE = np.dtype([("bmin", np.float32, 3), ("bmax", np.float32, 3), ("offset", np.int32), ("countAxis", np.uint32)])
assert EDGE.itemsize == 32 and CAND.itemsize == 32 and SCALARS.itemsize == 40 and BVHNODE.itemsize == 32
NODES = 64      # the first nodes of each build
PLANE = 33      # Cand.k of a plane candidate
CAPS = ("maxEdges", "maxFaces", "maxFaceEdges", "maxStack")


class DebugBspNode(C.Structure):
    """HprtDebugBspNode (csrc/capi_host.cpp)"""
    _fields_ = [("edges", C.c_void_p), ("n_edges", C.c_uint32), ("dirs", C.c_void_p), ("M", C.c_uint32), ("scalars", C.c_void_p),
                ("cands", C.c_void_p), ("n", C.c_size_t), ("n_axis", C.c_size_t), ("bvh_nodes", C.c_void_p), ("n_bvh", C.c_uint32),
                ("prim_order", C.c_void_p), ("prim_nums", C.c_void_p), ("n_prims", C.c_uint32),
                ("bmin", C.c_void_p), ("bmax", C.c_void_p), ("tri9", C.c_void_p), ("is_tri", C.c_void_p), ("n_total", C.c_size_t),
                ("costs", C.c_void_p), ("costs_fixed", C.c_void_p), ("level", C.c_uint32)]


SINK = C.CFUNCTYPE(None, C.c_void_p, C.c_uint32, C.POINTER(DebugBspNode))


def _copy(ptr, dtype, n):
    if n == 0 or not ptr:
        return np.zeros(0, dtype)
    return np.frombuffer(C.string_at(ptr, n * np.dtype(dtype).itemsize), dtype).copy()


def params(hprt, **kw):
    return hprt.BspPaperKdParams(kw.get("isect_cost", 80), kw.get("trav_cost", 5), kw.get("kd_trav_cost", 1), kw.get("empty_bonus", 0.0),
                                 kw.get("max_prims", 1), kw.get("max_depth", -1), 0)


def build_nodes(hprt, kd_aware, p9=None, model=None, max_nodes=NODES, **kw):
    """[dict] of the first max_nodes nodes the build costs; costs, costs_fixed and the candidates' counts: the builder's own.  The
    build's primitive arrays are shared by the nodes of one build."""
    out = []
    prims = {}

    def sink(user, index, ptr):
        nd = ptr.contents
        if not prims:
            prims.update(bmin=_copy(nd.bmin, np.float32, 3 * nd.n_total), bmax=_copy(nd.bmax, np.float32, 3 * nd.n_total),
                         tri9=_copy(nd.tri9, np.float32, 9 * nd.n_total), is_tri=_copy(nd.is_tri, np.uint8, nd.n_total))
        n_prims = nd.n_prims
        out.append(dict(kd_aware=kd_aware, level=nd.level, edges=_copy(nd.edges, EDGE, nd.n_edges), dirs=_copy(nd.dirs, np.float32, 3 * nd.M),
                        scalars=_copy(nd.scalars, SCALARS, 1), cands=_copy(nd.cands, CAND, nd.n), n_axis=nd.n_axis,
                        bvh=_copy(nd.bvh_nodes, BVHNODE, nd.n_bvh), prim_order=_copy(nd.prim_order, np.uint32, n_prims if nd.n_bvh else 0),
                        prim_nums=_copy(nd.prim_nums, np.uint32, n_prims), prims=prims, costs=_copy(nd.costs, np.float32, nd.n),
                        costs_fixed=_copy(nd.costs_fixed, np.float32, nd.n) if nd.costs_fixed else None))

    fn = hprt.lib.hprt_debug_bsp_root_nodes
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, SINK, C.c_void_p]
    cb = SINK(sink)
    prm = params(hprt, **kw)
    if model is not None:
        rc = fn(model._h, 0, None, int(kd_aware), C.byref(prm), max_nodes, cb, None)
    else:
        p9 = np.ascontiguousarray(p9, np.float32).reshape(-1, 9)
        rc = fn(None, p9.shape[0], p9.ctypes.data_as(C.c_void_p), int(kd_aware), C.byref(prm), max_nodes, cb, None)
    hprt._check(rc)
    return out


def cost(hprt, node, impl, cands=None, n_axis=None, zero_counts=True, **over):
    """(rc, costs, costs_fixed, counts [n, 2], overflow) of hprt_debug_bsp_cost over a node of build_nodes.  cands / n_axis: a
    sub-range of the node's candidates; zero_counts clears the plane candidates' counts first, so that what comes back is the
    costing's own; over: capacity fields of the scalars (CAPS), or replacements of the node's arrays (edges, dirs, bvh, prim_order,
    prim_nums, M)."""
    cands = np.ascontiguousarray((node["cands"] if cands is None else cands).copy())
    n_axis = int(node["n_axis"] if n_axis is None else n_axis)
    if zero_counts:
        pl = cands["k"] == PLANE
        cands["nBelow"][pl] = 0; cands["nAbove"][pl] = 0
    sc = node["scalars"].copy()
    for k in CAPS:
        sc[k] = over.pop(k, 0)
    arr = {k: np.ascontiguousarray(over.pop(k, node[k])) for k in ("edges", "dirs", "bvh", "prim_order", "prim_nums")}
    M = over.pop("M", arr["dirs"].shape[0] // 3)
    assert not over, over
    p = node["prims"]
    n = cands.shape[0]
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
    nd = DebugBspNode(vp(arr["edges"]), arr["edges"].shape[0], vp(arr["dirs"]), M, vp(sc), vp(cands), n, n_axis, vp(arr["bvh"]), arr["bvh"].shape[0],
                      vp(arr["prim_order"]), vp(arr["prim_nums"]), arr["prim_nums"].shape[0], vp(p["bmin"]), vp(p["bmax"]), vp(p["tri9"]),
                      vp(p["is_tri"]), p["is_tri"].shape[0], None, None, 0)
    costs = np.full(n, np.nan, np.float32); fixed = np.full(n, np.nan, np.float32)
    counts = np.full((n, 2), 0xdeadbeef, np.uint32); ovf = np.full(n, 255, np.uint8)
    fn = hprt.lib.hprt_debug_bsp_cost
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(DebugBspNode), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    rc = fn(C.byref(nd), int(node["kd_aware"]), impl, costs.ctypes.data_as(C.c_void_p), fixed.ctypes.data_as(C.c_void_p),
            counts.ctypes.data_as(C.c_void_p), ovf.ctypes.data_as(C.c_void_p))
    return rc, costs, fixed, counts, ovf


def builder_results(node):
    """(costs, costs_fixed, counts [n, 2]) as the builder's own code left them; costs_fixed +inf where the build keeps none"""
    c = node["cands"]
    fixed = node["costs_fixed"] if node["costs_fixed"] is not None else np.full(c.shape[0], np.inf, np.float32)
    return node["costs"], fixed, np.stack([c["nBelow"], c["nAbove"]], axis=1)


@functools.lru_cache(maxsize=None)
def _node_sets(key):
    import importlib
    hprt = importlib.import_module("thesis-pbrt-v3_amd")
    kind, kd = key
    if kind == "dodecahedron":
        return build_nodes(hprt, kd, model=hprt.Model.load(DODECA))
    n, name = kind
    return build_nodes(hprt, kd, p9=dict(soups(n))[name])


def node_sets():
    """the builds the issue names: the dodecahedron, the 300-triangle random soup and the 200-triangle grid-snapped soup, plain and
    kd-aware"""
    return [(kind, kd) for kind in ("dodecahedron", (300, "random"), (200, "grid1")) for kd in (False, True)]


def nodes_of(key):
    return _node_sets(key)


def equal_where(ok, a, b):
    """bit equality of float32 or uint32 arrays on the rows `ok`"""
    return np.array_equal(np.asarray(a)[ok].view(np.uint32), np.asarray(b)[ok].view(np.uint32))
