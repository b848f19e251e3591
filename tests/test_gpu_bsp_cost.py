"""k_bspcost (csrc/device/bsp_cost.hip) and the device-assisted BspPaper / BspPaperKd builds on the GPU: the kernel against
bsp_cost.h on the host on the candidates of real build nodes (tests/test_bsp_cost_host.py holds that to the builder's own code and
shows that no flag is set at the compiled capacities), whole trees against the host build, the repair path, both paths in one
tree, model builds with spheres, a device-built tree under the walk, the kernels' resources and the launcher's buffers over several
builds.  Every comparison is bit for bit."""
import os

import numpy as np
import pytest

import bsp_cost_nodes as B
from conftest import GOLDEN
from kdop_cost_nodes import soup
from tree_walk_checks import LIBHPRT, camera_rays, kernel_metadata

pytestmark = pytest.mark.gpu

# LDS = the mesh (BSP_MAX_EDGES * 32) + the direction list (3 * 72 floats) + the compact table (BSP_MAX_FACES / 2
# words) + the face list (BSP_MAX_FACE_EDGES bytes a lane) + the BVH stack (BSP_MAX_STACK words a lane; none in the kernels of the
# axis candidates, which walk no BVH)
LDS_AXIS = 64 * 32 + 72 * 12 + 24 * 4 + 32 * 64
LDS_PLANES = 64 * 32 + 72 * 12 + 24 * 4 + 32 * 64 + 32 * 4 * 64


def _same(hprt, nd, **kw):
    """impl 2 against impl 1 over nd: the same flags, and costs, fixed costs and counts wherever unflagged; returns the flags"""
    rc1, c1, f1, n1, o1 = B.cost(hprt, nd, 1, **kw)
    rc2, c2, f2, n2, o2 = B.cost(hprt, nd, 2, **kw)
    assert rc1 == 0 and rc2 == 0, (rc1, rc2)
    assert np.array_equal(o1, o2)
    ok = o2 == 0
    assert B.equal_where(ok, c1, c2) and B.equal_where(ok, f1, f2) and B.equal_where(ok, n1, n2)
    return o2


@pytest.mark.parametrize("key", B.node_sets(), ids=lambda k: (k[0] if isinstance(k[0], str) else "%s%d" % (k[0][1], k[0][0])) + ("-kd" if k[1] else ""))
def test_kernel_equals_the_host_restatement(hprt, key):
    """impl 2 == impl 1 — costs, fixed costs, counts and flags — on every candidate of the first 64 nodes; the flags are all zero"""
    sizes = []
    for nd in B.nodes_of(key):
        assert not _same(hprt, nd).any()
        sizes.append(len(nd["cands"]))
    assert max(sizes) > 64 and min(sizes) >= 1


def test_ragged_candidate_counts(hprt):
    """one candidate, counts below / at / above a wave and 64 k + 1; ranges of axis candidates only and of plane candidates only"""
    nd = B.nodes_of(((300, "random"), True))[0]
    na = int(nd["n_axis"])
    assert na > 193 and len(nd["cands"]) - na > 193
    for n in (1, 37, 63, 64, 65, 193):
        assert not _same(hprt, nd, cands=nd["cands"][:n], n_axis=n).any(), n                      # all axis candidates
        assert not _same(hprt, nd, cands=nd["cands"][na:na + n], n_axis=0).any(), n               # all plane candidates
        mixed = np.concatenate([nd["cands"][na - n:na], nd["cands"][na:na + n]])
        assert not _same(hprt, nd, cands=mixed, n_axis=n).any(), n


def test_deep_nodes_and_a_direction_that_owns_no_face(hprt):
    """nodes 8 levels down with grown direction lists, and the made-up nodes of tests/test_bsp_cost_host.py in which a direction
    without a face takes candidates"""
    from test_bsp_cost_host import _deep_nodes, faceless_direction_nodes
    deep = _deep_nodes(hprt, False)[:32] + _deep_nodes(hprt, True)[:32]
    made = faceless_direction_nodes(deep)
    assert len(deep) >= 8 and len(made) >= 4
    for nd in deep + made:
        assert not _same(hprt, nd).any()


def _model(hprt, tmp_path, shapes):
    from test_host_side import HEADER
    (tmp_path / "s.pbrt").write_text(HEADER + shapes + "WorldEnd\n")
    return hprt.Model.parse(str(tmp_path / "s.pbrt"))


def _spheres(n, seed):
    rng = np.random.default_rng(seed)
    return "".join('AttributeBegin Translate %r %r %r Shape "sphere" "float radius" [%r] AttributeEnd\n' % (*map(float, rng.uniform(-3, 3, 3)), float(rng.uniform(0.2, 0.9)))
                   for _ in range(n))


def test_a_node_of_spheres_only(hprt, tmp_path):
    """no primitive offers a plane: axis candidates only, no BVH"""
    m = _model(hprt, tmp_path, _spheres(24, 3))
    for kd in (False, True):
        nodes = B.build_nodes(hprt, kd, model=m, max_nodes=16)
        assert nodes and all(len(nd["bvh"]) == 0 and nd["n_axis"] == len(nd["cands"]) for nd in nodes)
        for nd in nodes:
            assert not _same(hprt, nd).any()
        dev = (hprt.BspPaperKd if kd else hprt.BspPaper)(m, isect_cost=80, device=0, min_candidates=1)
        _same_tree(dev, (hprt.BspPaperKd if kd else hprt.BspPaper)(m, isect_cost=80))
        assert dev.build_stats["nodes_device"] > 0 and dev.build_stats["candidates_recosted_on_host"] == 0


def test_spheres_among_triangles(hprt, tmp_path):
    """a straddling BVH leaf that holds a sphere projects the 8 corners of its bound"""
    p9 = dict(B.soups(200))["random"][:60] * np.float32(0.3)
    tris = 'Shape "trianglemesh" "integer indices" [%s] "point P" [%s]\n' % (" ".join(map(str, range(180))), " ".join(repr(float(v)) for v in p9.ravel()))
    m = _model(hprt, tmp_path, _spheres(12, 4) + tris)
    nodes = B.build_nodes(hprt, False, model=m, max_nodes=24)
    assert not nodes[0]["prims"]["is_tri"].all() and nodes[0]["prims"]["is_tri"].any()
    corners = 0
    for nd in nodes:
        assert not _same(hprt, nd).any()
        corners += int((nd["prims"]["is_tri"][nd["prim_nums"]] == 0).sum()) if len(nd["bvh"]) else 0
    assert corners > 0


LOWERED = (("maxEdges", 16), ("maxFaces", 10), ("maxFaceEdges", 5), ("maxStack", 4))


@pytest.mark.parametrize("field,value", LOWERED, ids=[f for f, _ in LOWERED])
def test_lowered_capacity_flags_the_same_candidates(hprt, field, value):
    """the kernel flags exactly what the host restatement flags, and agrees elsewhere"""
    flagged = 0
    for nd in B.nodes_of(((200, "grid1"), False)) + B.nodes_of(((300, "random"), True)):
        flagged += int(_same(hprt, nd, **{field: value}).sum())
    assert flagged > 0


def _same_tree(a, b):
    na, ia = a.arrays(); nb, ib = b.arrays()
    assert na.shape == nb.shape and np.array_equal(na, nb) and np.array_equal(ia, ib)
    assert a.info() == b.info()


@pytest.mark.parametrize("kd", [False, True], ids=["bsppaper", "bsppaperkd"])
def test_whole_trees_equal_the_host_build(hprt, kd):
    """200-triangle soups, plain and grid-snapped, every costed node through the kernel (min_candidates = 1)"""
    cls = hprt.BspPaperKd if kd else hprt.BspPaper
    for name, p9 in B.soups(200):
        dev = cls.from_triangles(p9, device=0, min_candidates=1)
        _same_tree(dev, cls.from_triangles(p9))
        st = dev.build_stats
        assert st["candidates_recosted_on_host"] == 0 and st["nodes_device"] > 0 and st["candidates_device"] > 0, (name, st)      # (nodes_host: nodes without a candidate)


def test_both_paths_meet_in_one_tree(hprt):
    """1,500 triangles on a grid with the default threshold: large nodes on the device, small ones on the host (maxprims 16 keeps
    both builds to a few seconds)"""
    p9 = soup(np.random.default_rng(5), 1500, grid=0.25, degenerate=0.05)
    dev = hprt.BspPaper.from_triangles(p9, max_prims=16, device=0)
    _same_tree(dev, hprt.BspPaper.from_triangles(p9, max_prims=16))
    st = dev.build_stats
    assert st["nodes_device"] > 0 and st["nodes_host"] > 0 and st["candidates_recosted_on_host"] == 0, st


def test_repair_path(hprt):
    """lowered capacities: flagged candidates, and whole nodes beyond them, are costed on the host; the tree is the same"""
    p9 = dict(B.soups(200))["grid1"]
    for cls in (hprt.BspPaper, hprt.BspPaperKd):
        host = cls.from_triangles(p9)
        for caps in (dict(max_edges=16), dict(max_faces=10, max_face_edges=5), dict(max_stack=4)):
            dev = cls.from_triangles(p9, device=0, min_candidates=1, **caps)
            _same_tree(dev, host)
            assert dev.build_stats["candidates_recosted_on_host"] > 0 and dev.build_stats["candidates_device"] > 0, (caps, dev.build_stats)
    with pytest.raises(hprt.HprtError) as e:
        hprt.BspPaper.from_triangles(p9, device=0, max_edges=4096)      # may only lower the capacity
    assert e.value.code == hprt.E_INVALID


def test_model_builds_equal_the_host_build(hprt, tmp_path_factory):
    from test_gpu_bsppaper import _prefix_scene
    m = hprt.Model.load(B.DODECA)
    for cls in (hprt.BspPaper, hprt.BspPaperKd):
        dev = cls(m, device=0, min_candidates=1)
        _same_tree(dev, cls(m))
        assert dev.build_stats["nodes_device"] > 0 and dev.build_stats["candidates_recosted_on_host"] == 0
    q = hprt.Model.load(_prefix_scene(tmp_path_factory, hprt))        # 2,000 triangles and three spheres
    dev = hprt.BspPaper(q, device=0)
    _same_tree(dev, hprt.BspPaper(q))
    assert dev.build_stats["nodes_device"] > 0 and dev.build_stats["candidates_recosted_on_host"] == 0, dev.build_stats


def test_a_device_built_tree_walks_like_the_host_built_one(hprt, orc):
    m = hprt.Model.load(B.DODECA)
    o, d, tm = camera_rays(np.random.default_rng(9), orc.OracleScene(B.DODECA), 4096)
    hits = []
    for tree in (hprt.BspPaper(m), hprt.BspPaper(m, device=0, min_candidates=1)):
        sc = hprt.Scene(m, hprt.Bvh(m), device=0)
        sc.attach_bsppaper(tree)
        hits.append(sc.intersect(o, d, tm, count=True))
    (t0, p0, b0, c0), (t1, p1, b1, c1) = hits
    assert (p0 >= 0).any() and (p0 < 0).any()      # some rays hit the dodecahedron, some pass it
    assert B.same_bits(t0, t1) and np.array_equal(p0, p1) and B.same_bits(b0, b1) and np.array_equal(c0, c1)


def test_kernel_resources(tmp_path):
    """wave64, the LDS DESIGN.md 8n states, nothing spilled, nothing in scratch"""
    ks = {n: k for n, k in kernel_metadata(LIBHPRT, tmp_path).items() if "k_bspcost" in n}
    assert len(ks) == 4 and sorted(n.split("k_bspcost")[1][:12] for n in ks) == ["ILb0ELb0EEEv", "ILb0ELb1EEEv", "ILb1ELb0EEEv", "ILb1ELb1EEEv"], sorted(ks)
    for n, k in ks.items():
        planes = "ELb1EEEv" in n
        assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, n
        assert k[".group_segment_fixed_size"] == (LDS_PLANES if planes else LDS_AXIS) and k[".private_segment_fixed_size"] == 0, (n, k[".group_segment_fixed_size"])
        assert k[".wavefront_size"] == 64 and k[".max_flat_workgroup_size"] == 64, n


def test_buffers_are_released_and_reused(hprt):
    """three builds in a row around a refused one (an instanced model), then a good one"""
    p9 = dict(B.soups(200))["random"]
    host = hprt.BspPaper.from_triangles(p9)
    inst = hprt.Model.load(os.path.join(GOLDEN, "simple_instanced.hprt"))
    _same_tree(hprt.BspPaper.from_triangles(p9, device=0, min_candidates=1), host)
    _same_tree(hprt.BspPaper.from_triangles(p9, device=0, min_candidates=1), host)
    with pytest.raises(hprt.HprtError) as e:
        hprt.BspPaper(inst, device=0, min_candidates=1)
    assert e.value.code == hprt.E_UNSUPPORTED
    _same_tree(hprt.BspPaper.from_triangles(p9, device=0, min_candidates=1), host)
    with pytest.raises(hprt.HprtError) as e:
        hprt.BspPaperKd(inst, device=0)
    assert e.value.code == hprt.E_UNSUPPORTED
    _same_tree(hprt.BspPaper.from_triangles(p9, device=0, min_candidates=1), host)
