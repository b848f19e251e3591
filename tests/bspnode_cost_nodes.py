"""Shared by tests/test_bspnode_cost_host.py and tests/test_gpu_bspnode_cost.py: the inputs of the node-based BSP candidate-costing
tests and thin wrappers over the two diagnostics hooks.  The nodes come from the builder itself (hprt_debug_bspnode_root_nodes hands
out the first nodes of a real build: mesh, the node's directions, the sweep's directions with their kinds and the candidates, with
the costs the builder's own code gave them); hprt_debug_bspnode_cost costs them again with impl 0 (the vector code), 1
(bspnode_cost.h on the host) or 2 (k_sweepcost).  The soups are those of tests/kdop_cost_nodes.py."""
import ctypes as C
import functools

import numpy as np

from bsp_cost_nodes import DODECA, EDGE, SCALARS, _copy, equal_where      # noqa: F401  (re-exported)
from kdop_cost_nodes import soups, same_bits      # noqa: F401

CAND = np.dtype([("k", np.uint32), ("nBelow", np.uint32), ("nAbove", np.uint32), ("t", np.float32)])
SWEEP = np.dtype([("axis", np.float32, 3), ("kind", np.uint32)])
assert CAND.itemsize == 16 and SWEEP.itemsize == 16
NODES = 64                                   # the first nodes of each build
PLAIN, KD_AXIS, CHOSEN = 0, 1, 2             # bspnodecost::KIND_*
MAX_SWEEP_DIRS = 16                          # BSPNODE_MAX_SWEEP_DIRS
CAPS = ("maxEdges", "maxFaces", "maxFaceEdges")
NAMES = tuple("bsp" + c + f for c in ("arbitrary", "cluster", "random") for f in ("", "withkd", "fastkd"))
FASTKD = tuple(n for n in NAMES if n.endswith("fastkd"))


class DebugSweepNode(C.Structure):
    """HprtDebugBspSweepNode (csrc/capi_host.cpp)"""
    _fields_ = [("edges", C.c_void_p), ("n_edges", C.c_uint32), ("dirs", C.c_void_p), ("M", C.c_uint32), ("sweep", C.c_void_p), ("n_dirs", C.c_uint32),
                ("scalars", C.c_void_p), ("cands", C.c_void_p), ("n", C.c_size_t), ("costs", C.c_void_p), ("costs_fixed", C.c_void_p), ("level", C.c_uint32)]


SINK = C.CFUNCTYPE(None, C.c_void_p, C.c_uint32, C.POINTER(DebugSweepNode))


def params(hprt, name, K, seed=5489, **kw):
    k = NAMES.index(name)
    return hprt.BspNodeParams(k // 3, k % 3, K, seed, kw.get("isect_cost", 80), kw.get("trav_cost", 5), kw.get("kd_trav_cost", 1), kw.get("empty_bonus", 0.0),
                              kw.get("max_prims", 1), kw.get("max_depth", -1), 0)


def build_nodes(hprt, name, K, p9=None, model=None, max_nodes=NODES, seed=5489, **kw):
    """[dict] of the first max_nodes nodes the build of accelerator `name` with K directions costs; costs and costs_fixed: the
    builder's own"""
    out = []
    fastkd = name.endswith("fastkd")

    def sink(user, index, ptr):
        nd = ptr.contents
        out.append(dict(fastkd=fastkd, level=nd.level, edges=_copy(nd.edges, EDGE, nd.n_edges), dirs=_copy(nd.dirs, np.float32, 3 * nd.M),
                        sweep=_copy(nd.sweep, SWEEP, nd.n_dirs), scalars=_copy(nd.scalars, SCALARS, 1), cands=_copy(nd.cands, CAND, nd.n),
                        costs=_copy(nd.costs, np.float32, nd.n), costs_fixed=_copy(nd.costs_fixed, np.float32, nd.n) if nd.costs_fixed else None))

    fn = hprt.lib.hprt_debug_bspnode_root_nodes
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint32, SINK, C.c_void_p]
    cb = SINK(sink)
    prm = params(hprt, name, K, seed, **kw)
    if model is not None:
        rc = fn(model._h, 0, None, C.byref(prm), max_nodes, cb, None)
    else:
        p9 = np.ascontiguousarray(p9, np.float32).reshape(-1, 9)
        rc = fn(None, p9.shape[0], p9.ctypes.data_as(C.c_void_p), C.byref(prm), max_nodes, cb, None)
    hprt._check(rc)
    return out


def cost(hprt, node, impl, cands=None, **over):
    """(rc, costs, costs_fixed, overflow, declined) of hprt_debug_bspnode_cost over a node of build_nodes.  cands: a sub-range of
    the node's candidates; over: capacity fields of the scalars (CAPS), or replacements of the node's arrays (edges, dirs, sweep,
    M, fastkd)."""
    cands = np.ascontiguousarray((node["cands"] if cands is None else cands).copy())
    sc = node["scalars"].copy()
    sc["maxStack"] = 0
    for k in CAPS:
        sc[k] = over.pop(k, 0)
    arr = {k: np.ascontiguousarray(over.pop(k, node[k])) for k in ("edges", "dirs", "sweep")}
    M = over.pop("M", arr["dirs"].shape[0] // 3)
    fastkd = over.pop("fastkd", node["fastkd"])
    assert not over, over
    n = cands.shape[0]
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
    nd = DebugSweepNode(vp(arr["edges"]), arr["edges"].shape[0], vp(arr["dirs"]), M, vp(arr["sweep"]), arr["sweep"].shape[0], vp(sc), vp(cands), n, None, None, 0)
    costs = np.full(n, np.nan, np.float32); fixed = np.full(n, np.nan, np.float32)
    ovf = np.full(n, 255, np.uint8)
    declined = C.c_int(-1)
    fn = hprt.lib.hprt_debug_bspnode_cost
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(DebugSweepNode), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
    rc = fn(C.byref(nd), int(fastkd), impl, costs.ctypes.data_as(C.c_void_p), fixed.ctypes.data_as(C.c_void_p), ovf.ctypes.data_as(C.c_void_p),
            C.byref(declined))
    return rc, costs, fixed, ovf, declined.value


def builder_results(node):
    """(costs, costs_fixed) as the builder's own code left them; costs_fixed +inf where the build keeps none"""
    fixed = node["costs_fixed"] if node["costs_fixed"] is not None else np.full(node["cands"].shape[0], np.inf, np.float32)
    return node["costs"], fixed


def input_of(hprt, kind):
    """dict(model=...) or dict(p9=...) of an input's name: "dodecahedron" or (n, soup name)"""
    if kind == "dodecahedron":
        return dict(model=hprt.Model.load(DODECA))
    return dict(p9=dict(soups(kind[0]))[kind[1]])


@functools.lru_cache(maxsize=None)
def _node_sets(key):
    import importlib
    hprt = importlib.import_module("thesis-pbrt-v3_amd")
    kind, name, K = key
    return build_nodes(hprt, name, K, **input_of(hprt, kind))


INPUTS = ("dodecahedron", (200, "random"), (300, "grid1"))


def node_sets():
    """the builds the issue names: all nine accelerators at K = 4 and the three fastkd ones also at K = 6, over the dodecahedron,
    the 200-triangle random soup and the 300-triangle grid-snapped soup"""
    return [(kind, name, K) for kind in INPUTS for name, K in [(n, 4) for n in NAMES] + [(n, 6) for n in FASTKD]]


def set_id(key):
    kind, name, K = key
    return "%s-%s-%d" % (kind if isinstance(kind, str) else "%s%d" % (kind[1], kind[0]), name, K)


def nodes_of(key):
    return _node_sets(key)
