"""k_sweepcost (csrc/device/bspnode_cost.hip) and the device-assisted node-based BSP builds on the GPU: the kernel against
bspnode_cost.h on the host on the candidates of real build nodes (tests/test_bspnode_cost_host.py holds that to the builder's own
code and shows that no flag is set at the compiled capacities), whole trees against the host build, the repair path, declined
nodes, both paths in one tree, a model with spheres, a device-built tree under the walk, the kernels' resources and the launcher's
buffers over several builds.  Every comparison is bit for bit."""
import numpy as np
import pytest

import bspnode_cost_nodes as B
from tree_walk_checks import LIBHPRT, camera_rays, kernel_metadata

pytestmark = pytest.mark.gpu

# LDS = the mesh (BSP_MAX_EDGES * 32) + the node's direction list (3 * 72 floats) + the compact table (BSP_MAX_FACES / 2
# words) + the face list (BSP_MAX_FACE_EDGES bytes a lane) + the per-direction table (BSPNODE_MAX_SWEEP_DIRS * 32)
LDS = 64 * 32 + 72 * 12 + 24 * 4 + 32 * 64 + 16 * 32


def same(hprt, nd, cands=None, **kw):
    """impl 2 against impl 1 over nd: the same flags and decline, and costs and fixed costs wherever unflagged; returns the flags"""
    rc1, c1, f1, o1, d1 = B.cost(hprt, nd, 1, cands=cands, **kw)
    rc2, c2, f2, o2, d2 = B.cost(hprt, nd, 2, cands=cands, **kw)
    assert rc1 == 0 and rc2 == 0, (rc1, rc2)
    assert d1 == d2 and np.array_equal(o1, o2)
    ok = o2 == 0
    assert B.equal_where(ok, c1, c2) and B.equal_where(ok, f1, f2)
    return o2


@pytest.mark.parametrize("key", B.node_sets(), ids=B.set_id)
def test_kernel_equals_the_host_restatement(hprt, key):
    """impl 2 == impl 1 — costs, fixed costs and flags — on every candidate of the first 64 nodes; the flags are all zero"""
    sizes = []
    for nd in B.nodes_of(key):
        assert not same(hprt, nd).any()
        sizes.append(len(nd["cands"]))
    assert max(sizes) > 64 and min(sizes) >= 1


def test_ragged_candidate_ranges(hprt):
    """one candidate, counts below / at / above a wave and 64 k + 1: ranges that begin and end inside a direction, ranges of kd
    axes only and of chosen directions only"""
    nd = B.nodes_of(((300, "grid1"), "bspclusterfastkd", 6))[0]
    c = nd["cands"]
    kind = nd["sweep"]["kind"][c["k"]]
    axes, chosen = np.nonzero(kind == B.KD_AXIS)[0], np.nonzero(kind == B.CHOSEN)[0]
    first_chosen = int(chosen[0])
    assert len(axes) > 400 and len(chosen) > 400 and (axes < first_chosen).all()
    inside = int(np.nonzero(c["k"] == 1)[0][5])                       # a few candidates into the second axis
    assert (c["k"][inside:inside + 193] == 1).all()
    for n in (1, 37, 63, 64, 65, 193):
        across = first_chosen - n // 2 - 1                           # a range over the last axis and the first chosen direction
        ranges = (c[inside:inside + n], c[across:across + n], c[axes[-n:]], c[chosen[7:7 + n]])      # ..., kd axes only, chosen only
        for r in ranges:
            assert len(r) == n and not same(hprt, nd, cands=r).any(), n


def test_deep_nodes_and_the_odd_direction_sets(hprt, tmp_path):
    """nodes 8 levels down with grown direction lists, a sweep direction that owns no face, and the direction sets of
    tests/test_bspnode_cost_host.py: fastkd with K = 3, plain with K = 1, np <= K, equal directions, a zero direction, spheres"""
    from test_bspnode_cost_host import deep_nodes, faceless_direction_nodes, odd_direction_sets
    deep = deep_nodes(hprt, "bsprandom")[:24] + deep_nodes(hprt, "bsprandomfastkd")[:24]
    made = faceless_direction_nodes(deep)
    assert len(deep) >= 8 and len(made) >= 4
    for nd in deep + made:
        assert not same(hprt, nd).any()
    for label, nodes in odd_direction_sets(hprt, tmp_path).items():
        for nd in nodes:
            assert not same(hprt, nd).any(), label


LOWERED = (("maxEdges", 16), ("maxFaces", 10), ("maxFaceEdges", 5))


@pytest.mark.parametrize("field,value", LOWERED, ids=[f for f, _ in LOWERED])
def test_lowered_capacity_flags_the_same_candidates(hprt, field, value):
    """the kernel flags exactly what the host restatement flags, and agrees elsewhere"""
    from test_bspnode_cost_host import LOWERED_SETS
    flagged = 0
    for key in LOWERED_SETS:
        for nd in B.nodes_of(key):
            flagged += int(same(hprt, nd, **{field: value}).sum())
    assert flagged > 0


def test_a_sweep_beyond_the_direction_table_is_declined(hprt):
    nodes = B.build_nodes(hprt, "bsprandom", B.MAX_SWEEP_DIRS + 1, p9=dict(B.soups(200))["random"][:40], max_nodes=2)
    for nd in nodes:
        rc, c, f, o, d = B.cost(hprt, nd, 2)
        assert rc == 0 and d == 1 and o.all()


def same_tree(a, b):
    na, ia = a.arrays(); nb, ib = b.arrays()
    assert na.shape == nb.shape and np.array_equal(na, nb) and np.array_equal(ia, ib)
    assert a.info() == b.info()


def build(hprt, name, kind, K=4, seed=5489, **kw):
    """the tree of accelerator `name` over an input of bspnode_cost_nodes.input_of"""
    cls = hprt.BspNodeKd if name.endswith("fastkd") else hprt.BspNode
    src = B.input_of(hprt, kind)
    if "model" in src:
        return cls(src["model"], name, n_directions=K, seed=seed, **kw)
    return cls.from_triangles(src["p9"], name, n_directions=K, seed=seed, **kw)


_HOST = {}


def host_tree(hprt, name, kind, seed=5489):
    """the host build at K = 4, built once and shared by the tests that compare against it"""
    key = (name, kind, seed)
    if key not in _HOST:
        _HOST[key] = build(hprt, name, kind, seed=seed)
    return _HOST[key]


@pytest.mark.parametrize("name", B.NAMES)
def test_whole_trees_equal_the_host_build(hprt, name):
    """the dodecahedron and the 300-triangle random soup, seeds 5489 and 7, every costed node through the kernel
    (min_candidates = 1): nodes, axes, primIndices, bounds and counts"""
    for kind in ("dodecahedron", (300, "random")):
        for seed in (5489, 7):
            dev = build(hprt, name, kind, seed=seed, device=0, min_candidates=1)
            same_tree(dev, host_tree(hprt, name, kind, seed))
            st = dev.build_stats
            assert st["nodes_device"] > 0 and st["candidates_device"] > 0 and st["candidates_recosted_on_host"] == 0, (kind, seed, st)


@pytest.mark.parametrize("name", B.NAMES)
def test_repair_path(hprt, name):
    """the same builds with max_edges = 16: flagged candidates, and whole nodes beyond it, are costed on the host; the tree is the
    same.  (Every one of the 36 builds flags candidates of nodes that fit: 262 to 9,471 of them, counted with the restatement.)"""
    for kind in ("dodecahedron", (300, "random")):
        for seed in (5489, 7):
            dev = build(hprt, name, kind, seed=seed, device=0, min_candidates=1, max_edges=16)
            same_tree(dev, host_tree(hprt, name, kind, seed))
            st = dev.build_stats
            assert st["candidates_recosted_on_host"] > 0 and st["candidates_device"] > 0 and st["nodes_device"] > 0, (kind, seed, st)
    with pytest.raises(hprt.HprtError) as e:
        build(hprt, name, "dodecahedron", device=0, max_edges=4096)      # may only lower the capacity
    assert e.value.code == hprt.E_INVALID


@pytest.mark.parametrize("name", ("bspcluster", "bsprandomfastkd"))
def test_every_node_declined(hprt, name):
    """max_edges below the root's 12 edges, and below the 6 of the smallest polyhedron a deep node can be: no node fits, every one
    takes the host path"""
    dev = build(hprt, name, (300, "random"), device=0, min_candidates=1, max_edges=1)
    same_tree(dev, host_tree(hprt, name, (300, "random")))
    st = dev.build_stats
    assert st["nodes_device"] == 0 and st["candidates_device"] == 0 and st["candidates_recosted_on_host"] == 0 and st["nodes_host"] > 0, st


@pytest.mark.parametrize("name", ("bsparbitrary", "bspclusterfastkd"))
def test_both_paths_meet_in_one_tree(hprt, name):
    """a threshold between the root's candidates and a leaf's: large nodes on the device, small ones on the host"""
    dev = build(hprt, name, (300, "random"), device=0, min_candidates=200)
    same_tree(dev, host_tree(hprt, name, (300, "random")))
    st = dev.build_stats
    assert st["nodes_device"] > 0 and st["nodes_host"] > 0 and st["candidates_recosted_on_host"] == 0, st


def test_spheres_among_triangles(hprt, tmp_path):
    from test_bspnode_cost_host import sphere_model
    m = sphere_model(hprt, tmp_path)
    for cls, acc in ((hprt.BspNode, "bspcluster"), (hprt.BspNode, "bsparbitrarywithkd"), (hprt.BspNodeKd, "bsprandomfastkd")):
        dev = cls(m, acc, n_directions=5, device=0, min_candidates=1)
        same_tree(dev, cls(m, acc, n_directions=5))
        assert dev.build_stats["nodes_device"] > 0 and dev.build_stats["candidates_recosted_on_host"] == 0
    tree, attach = hprt.bspnode_tree(m, "bspclusterfastkd", n_directions=5, device=0, min_candidates=1)
    assert attach == "attach_bsppaperkd" and tree.build_stats["nodes_device"] > 0
    same_tree(tree, hprt.bspnode_tree(m, "bspclusterfastkd", n_directions=5)[0])


def test_a_device_built_tree_under_the_walk(hprt, orc):
    """a device-built bspclusterfastkd tree attached: camera rays through k_bsppaperkdwalk against the restated walk over the
    restated build"""
    import bspnode_ref as nref
    import tree_walk_checks as twc
    K, seed = 5, 7
    m = hprt.Model.load(B.DODECA)
    tree = hprt.BspNodeKd(m, "bspclusterfastkd", n_directions=K, seed=seed, device=0, min_candidates=1)
    assert tree.build_stats["nodes_device"] > 0
    ref = nref.NodeScene(B.DODECA, "bspclusterfastkd", K, seed)
    nref.assert_same_tree(tree.arrays(), ref.tree(), True)
    sc = hprt.Scene(m, hprt.Bvh(m), device=0)
    sc.attach_bsppaperkd(tree)
    twc.check_closest(sc, ref, [camera_rays(np.random.default_rng(9), orc.OracleScene(B.DODECA), 4096)])


def test_kernel_resources(tmp_path):
    """wave64, the LDS DESIGN.md 8o derives from the capacities, nothing spilled, nothing in scratch"""
    ks = {n: k for n, k in kernel_metadata(LIBHPRT, tmp_path).items() if "k_sweepcost" in n}
    assert len(ks) == 2 and sorted(n.split("k_sweepcost")[1][:8] for n in ks) == ["ILb0EEEv", "ILb1EEEv"], sorted(ks)
    for n, k in ks.items():
        assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, n
        assert k[".group_segment_fixed_size"] == LDS and k[".private_segment_fixed_size"] == 0, (n, k[".group_segment_fixed_size"])
        assert k[".wavefront_size"] == 64 and k[".max_flat_workgroup_size"] == 64, n


def test_buffers_are_released_and_reused(hprt):
    """a refused build (withkd, K = 2), then three good builds in a row"""
    p9 = dict(B.soups(200))["random"]
    with pytest.raises(hprt.HprtError) as e:
        hprt.BspNode.from_triangles(p9, "bspclusterwithkd", n_directions=2, device=0, min_candidates=1)
    assert e.value.code == hprt.E_UNSUPPORTED
    with pytest.raises(hprt.HprtError) as h:
        hprt.BspNode.from_triangles(p9, "bspclusterwithkd", n_directions=2)
    assert str(e.value) == str(h.value)                # the host entry's message
    host = hprt.BspNode.from_triangles(p9, "bspclusterwithkd", n_directions=4)
    for _ in range(3):
        same_tree(hprt.BspNode.from_triangles(p9, "bspclusterwithkd", n_directions=4, device=0, min_candidates=1), host)
