"""kdop_cost.h on the host: the fixed-capacity restatement of KDOPCut + KDOPSurfaceArea + the cost formulas against the vector code
of kdop_mesh.h, bit for bit, on the candidates of real build nodes (handed out by the builder itself); the overflow flags at the
default and at a lowered capacity; the validation of the diagnostics hook; the device entries without a device.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import kdop_cost_nodes as K


def _ids(k):
    return "%s-M%d%s" % (k[0], k[1], "-kd" if k[2] else "")


@pytest.mark.parametrize("key", K.node_sets(), ids=_ids)
def test_restatement_equals_the_vector_code(hprt, key):
    """impl 1 == impl 0 == the costs the builder's own costRange gave, on every candidate of the first 64 nodes; no flag is set
    at the default capacity, so nothing here passes by falling back"""
    nodes = K.nodes_of(key)
    assert len(nodes) == K.NODES
    total = 0
    for nd in nodes:
        rc0, c0, f0, o0 = K.cost(hprt, nd, 0)
        rc1, c1, f1, o1 = K.cost(hprt, nd, 1)
        assert rc0 == 0 and rc1 == 0 and not o0.any() and not o1.any()
        assert K.same_bits(c0, nd["costs"])
        assert K.same_bits(c0, c1) and K.same_bits(f0, f1)
        if key[2]:
            ob = nd["cands"]["d"] >= 3      # the builder writes costsFixed for oblique candidates only
            assert K.same_bits(f0[ob], nd["costs_fixed"][ob])
        total += len(c0)
    assert total > 1000


def test_lowered_capacity_flags_and_never_lies(hprt):
    """max_edges = 16 at M = 13: some candidates are flagged; an unflagged one carries the vector code's cost"""
    flagged = clean = 0
    for key in (("grid1", 13, False), ("grid1", 13, True), ("random", 13, False)):
        for nd in K.nodes_of(key):
            rc, c1, f1, o1 = K.cost(hprt, nd, 1, max_edges=16)
            assert rc == 0 and set(np.unique(o1)) <= {0, 1}
            ok = o1 == 0
            assert K.same_bits(c1[ok], nd["costs"][ok])
            if len(nd["edges"]) > 16:
                assert o1.all()      # a node's mesh beyond the capacity is not costed at all
            flagged += int(o1.sum()); clean += int(ok.sum())
    assert flagged > 0 and clean > 0


def test_debug_hook_rejects_malformed_input(hprt):
    nd = K.nodes_of(("random", 7, False))[0]
    E = hprt.E_INVALID
    for impl in (0, 1):
        assert K.cost(hprt, nd, impl)[0] == 0
        for M in (0, 5, 14, 26):
            assert K.cost(hprt, nd, impl, M=M)[0] == E
        bad = nd["edges"].copy(); bad["f1"][3] = 14                      # 2 M = 14
        assert K.cost(hprt, nd, impl, edges=bad)[0] == E
        bad = nd["edges"].copy(); bad["f2"][0] = 0xffffffff
        assert K.cost(hprt, nd, impl, edges=bad)[0] == E
        bad = nd["cands"].copy(); bad["d"][-1] = 7
        assert K.cost(hprt, nd, impl, cands=bad)[0] == E
        assert K.cost(hprt, nd, impl, max_edges=4096)[0] == E            # may only lower the capacity
    assert K.cost(hprt, nd, 3)[0] == E and K.cost(hprt, nd, -1)[0] == E
    fn = hprt.lib.hprt_debug_kdop_cost
    assert fn(None, 1, 7, 0, None, None, 0, 1, None, None, None) == E
    # a mesh of more edges than the capacity: valid input, every candidate flagged, nothing costed
    big = np.concatenate([nd["edges"]] * 6)
    assert len(big) > 48
    rc, c, f, o = K.cost(hprt, nd, 1, edges=big)
    assert rc == 0 and o.all()


def test_device_entries_without_a_device(hprt):
    """hprt_*_build*_device: HPRT_E_NO_DEVICE and *out NULL where there is no HIP device; the host refusals come first"""
    import torch
    p9 = dict(K.soups(200))["random"]
    fn = hprt.lib.hprt_rbsp_build_from_triangles_device
    prm = hprt.RbspParams(80, 5, 0.0, 1, -1, 7, 0)
    h = C.c_void_p(0xdead)
    st = hprt.BuildDeviceStats()
    rc = fn(p9.shape[0], p9.ctypes.data_as(C.c_void_p), C.byref(prm), None, C.byref(st), C.byref(h))
    if torch.cuda.is_available():
        assert rc == 0 and h.value
        hprt.lib.hprt_rbsp_destroy(h)
    else:
        assert rc == hprt.E_NO_DEVICE and h.value is None
        kh = C.c_void_p(0xdead)
        kprm = hprt.RbspKdParams(80, 5, 1, 0.0, 1, -1, 7, 0)
        assert hprt.lib.hprt_rbspkd_build_from_triangles_device(p9.shape[0], p9.ctypes.data_as(C.c_void_p), C.byref(kprm), None, None, C.byref(kh)) == hprt.E_NO_DEVICE
        assert kh.value is None
        with pytest.raises(hprt.HprtError) as e:
            hprt.Rbsp(hprt.Model.load(K.DODECA), n_directions=7, device=0)
        assert e.value.code == hprt.E_NO_DEVICE
    bad = hprt.RbspParams(80, 5, 0.0, 1, -1, 5, 0)
    h = C.c_void_p(0xdead)
    assert fn(p9.shape[0], p9.ctypes.data_as(C.c_void_p), C.byref(bad), None, None, C.byref(h)) == hprt.E_UNSUPPORTED and h.value is None
