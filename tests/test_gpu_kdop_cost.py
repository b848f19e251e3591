"""k_kdopcost (csrc/device/kdop_cost.hip) and the device-assisted RBSP / RBSPKd builds on the GPU: the kernel against kdop_cost.h on
the host on the candidates of real build nodes, whole trees against the host build, the repair path, both paths in one tree, the
kernels' resources and the launcher's workspace over several builds.  Every comparison is bit for bit."""
import numpy as np
import pytest

import kdop_cost_nodes as K
from tree_walk_checks import LIBHPRT, kernel_metadata

pytestmark = pytest.mark.gpu

# LDS = the mesh (KDOP_MAX_EDGES * 32) + the direction table (39 floats) + the face list (32 bytes a lane)
LDS_BYTES = 3740
PRIVATE_BYTES = 0


@pytest.mark.parametrize("key", K.node_sets(), ids=lambda k: "%s-M%d%s" % (k[0], k[1], "-kd" if k[2] else ""))
def test_kernel_equals_the_host_restatement(hprt, key):
    """impl 2 == impl 1, costs and flags, on every candidate of the first 64 nodes; the flags are all zero, so nothing fell back"""
    sizes = []
    for nd in K.nodes_of(key):
        rc1, c1, f1, o1 = K.cost(hprt, nd, 1)
        rc2, c2, f2, o2 = K.cost(hprt, nd, 2)
        assert rc1 == 0 and rc2 == 0
        assert np.array_equal(o1, o2) and not o2.any()
        assert K.same_bits(c1, c2) and K.same_bits(f1, f2)
        sizes.append(len(c1))
    assert max(sizes) > 64 and min(sizes) >= 1


def test_ragged_candidate_counts(hprt):
    """fewer than 64 candidates, exactly 64 k + 1, one, and a count below / at / above a wave"""
    nd = K.nodes_of(("grid1", 13, False))[0]
    assert len(nd["cands"]) > 64 * 3 + 1
    _, c1, f1, o1 = K.cost(hprt, nd, 1)
    for n in (1, 37, 63, 64, 65, 64 * 3 + 1):
        rc, c2, f2, o2 = K.cost(hprt, nd, 2, cands=nd["cands"][:n])
        assert rc == 0 and K.same_bits(c2, c1[:n]) and np.array_equal(o2, o1[:n]), n
    small = [x for x in K.nodes_of(("dodecahedron", 3, False)) if 0 < len(x["cands"]) < 64]
    assert small
    rc, c2, _, o2 = K.cost(hprt, small[0], 2)
    assert rc == 0 and K.same_bits(c2, small[0]["costs"]) and not o2.any()


def test_lowered_capacity_flags_the_same_candidates(hprt):
    """max_edges = 16 at M = 13: the kernel flags what the host restatement flags, and agrees where neither does"""
    flagged = 0
    for nd in K.nodes_of(("grid1", 13, False))[:16]:
        _, c1, f1, o1 = K.cost(hprt, nd, 1, max_edges=16)
        rc, c2, f2, o2 = K.cost(hprt, nd, 2, max_edges=16)
        assert rc == 0 and np.array_equal(o1, o2)
        ok = o2 == 0
        assert K.same_bits(c1[ok], c2[ok]) and K.same_bits(nd["costs"][ok], c2[ok])
        flagged += int(o2.sum())
    assert flagged > 0


def _same_tree(a, b):
    na, ia = a.arrays(); nb, ib = b.arrays()
    assert na.shape == nb.shape and np.array_equal(na, nb) and np.array_equal(ia, ib)
    assert K.same_bits(a.directions(), b.directions())


@pytest.mark.parametrize("kd", [False, True], ids=["rbsp", "rbspkd"])
@pytest.mark.parametrize("M", K.MS)
def test_whole_trees_equal_the_host_build(hprt, M, kd):
    """200-triangle soups, plain and grid-snapped, every interior node through the kernel (min_candidates = 1)"""
    cls = hprt.RbspKd if kd else hprt.Rbsp
    for name, p9 in K.soups(200):
        dev = cls.from_triangles(p9, M, device=0, min_candidates=1)
        _same_tree(dev, cls.from_triangles(p9, M))
        st = dev.build_stats
        assert st["candidates_recosted_on_host"] == 0 and st["nodes_device"] > 0 and st["candidates_device"] > 0, (name, st)


def test_both_paths_meet_in_one_tree(hprt):
    """4,000 triangles on a grid at M = 13 with the default threshold: large nodes on the device, small ones on the host
    (maxprims 32 keeps the two builds to a few seconds: about 600 nodes of 1,024 candidates or more, 1,600 below)"""
    p9 = K.soup(np.random.default_rng(5), 4000, grid=0.25, degenerate=0.05)
    dev = hprt.Rbsp.from_triangles(p9, 13, max_prims=32, device=0)
    _same_tree(dev, hprt.Rbsp.from_triangles(p9, 13, max_prims=32))
    st = dev.build_stats
    assert st["nodes_device"] > 0 and st["nodes_host"] > 0 and st["candidates_recosted_on_host"] == 0, st


def test_repair_path(hprt):
    """max_edges = 16: flagged candidates (and whole nodes of more than 16 edges) are costed on the host; the tree is the same"""
    p9 = dict(K.soups(200))["grid1"]
    for cls in (hprt.Rbsp, hprt.RbspKd):
        dev = cls.from_triangles(p9, 13, device=0, min_candidates=1, max_edges=16)
        _same_tree(dev, cls.from_triangles(p9, 13))
        assert dev.build_stats["candidates_recosted_on_host"] > 0 and dev.build_stats["candidates_device"] > 0, dev.build_stats


def test_model_build_equals_the_host_build(hprt):
    m = hprt.Model.load(K.DODECA)
    for M in (7, 13):
        dev = hprt.Rbsp(m, n_directions=M, device=0, min_candidates=1)
        _same_tree(dev, hprt.Rbsp(m, n_directions=M))
        assert dev.build_stats["nodes_device"] > 0
        devk = hprt.RbspKd(m, n_directions=M, device=0, min_candidates=1)
        _same_tree(devk, hprt.RbspKd(m, n_directions=M))


def test_kernel_resources(tmp_path):
    ks = {n: k for n, k in kernel_metadata(LIBHPRT, tmp_path).items() if "k_kdopcost" in n}
    assert len(ks) == 2 and any("ILb1E" in n for n in ks) and any("ILb0E" in n for n in ks), sorted(ks)
    for n, k in ks.items():
        assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, n
        assert k[".group_segment_fixed_size"] == LDS_BYTES and k[".private_segment_fixed_size"] == PRIVATE_BYTES, n
        assert k[".vgpr_count"] <= 80 and k[".wavefront_size"] == 64, n


def test_workspace_is_released_and_reused(hprt):
    """two builds in a row, a refused one (unsupported M), then a good one"""
    p9 = dict(K.soups(200))["random"]
    host = hprt.Rbsp.from_triangles(p9, 7)
    _same_tree(hprt.Rbsp.from_triangles(p9, 7, device=0, min_candidates=1), host)
    _same_tree(hprt.Rbsp.from_triangles(p9, 7, device=0, min_candidates=1), host)
    with pytest.raises(hprt.HprtError) as e:
        hprt.Rbsp.from_triangles(p9, 5, device=0, min_candidates=1)
    assert e.value.code == hprt.E_UNSUPPORTED
    _same_tree(hprt.Rbsp.from_triangles(p9, 7, device=0, min_candidates=1), host)
