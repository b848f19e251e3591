"""Two-level RBSP trees on the host (hprt_rbspinst_*): what the already pinned RBSP builder is FED — every object's primitives in
object space, the top level's with an instance as a non-triangle bounded by TransformedPrimitive::WorldBound, the parameters of the
Accelerator line per tree — the handle's info and copies, the refusals, the depth rule, and that the existing rbsp entry points and
warnings stay as they are."""
import numpy as np
import pytest

import deep_todo
import rbspinst_ref
import rbspinst_scenes as rs

PARAMS = ' "integer maxprims" [2] "float emptybonus" [0.2] "integer intersectcost" [40] "integer traversalcost" [3]'
KW = dict(max_prims=2, empty_bonus=0.2, isect_cost=40, trav_cost=3)


def _off(M):
    return int(M).bit_length()


@pytest.fixture(scope="module", params=[(kd, M, p) for kd in (False, True) for M in (3, 13) for p in ("defaults", "parameters")],
                ids=lambda c: "%s-%d-%s" % ("rbspkd" if c[0] else "rbsp", c[1], c[2]))
def built(request, hprt, tmp_path_factory):
    kd, M, which = request.param
    with_params = which == "parameters"
    m, path = rs.bake(hprt, tmp_path_factory.mktemp("rbspinst"), rs.scene_text(kd, M, PARAMS if with_params else ""), "scene")
    return m, hprt.RbspInst(m, kd_aware=kd), rbspinst_ref.RbspInstScene(path, M, kd), (KW if with_params else {}), kd, M


def _depth(nodes, M):
    """interior levels of the deepest path"""
    off, mask = _off(M), (1 << _off(M)) - 1

    def rec(k):
        if nodes[k, 1] & mask == M:
            return 0
        return 1 + max(rec(k + 1), rec(int(nodes[k, 1] >> off)))
    return rec(0)


def test_the_triangle_objects_tree_is_the_pinned_builders_over_its_object_space_triangles(hprt, built):
    m, ri, ref, kw, kd, M = built
    tri, p9, lo, hi = ref.prims(0)
    assert tri.all() and p9.shape == (20, 9) and p9.tobytes() == rs.blob_triangles().tobytes()
    want = (hprt.RbspKd if kd else hprt.Rbsp).from_triangles(p9, n_directions=M, **kw)
    nodes, idx = ri.object_copy(0)
    wn, wi = want.arrays()
    assert nodes.tobytes() == wn.tobytes() and idx.tobytes() == wi.tobytes()
    assert ri.object_info(0)["depth"] == want.info()["depth"] and ri.object_info(0)["leaves"] == want.info()["leaves"]
    assert ri.directions().tobytes() == want.directions().tobytes()


def test_the_top_level_and_the_mixed_objects_trees_are_the_restated_builds_over_the_restatements_lists(built):
    m, ri, ref, kw, kd, M = built
    assert (ref.n_top, ref.n_objects, ref.n_instances) == (2 + 1 + 6, 3, 6)
    tri, _, _, _ = ref.prims(-1)
    assert tri.tolist() == [1, 1, 0] + [0] * 6                     # floor triangles, the sphere, six instances
    tri, p9, _, _ = ref.prims(2)
    assert tri.tolist() == [0, 1, 1] and not p9[0].any()             # the sphere has no vertices
    for obj in (-1, 2):
        wn, wi, wb = ref.build(obj, **kw)
        nodes, idx = ri.copy() if obj < 0 else ri.object_copy(obj)
        assert nodes.tobytes() == wn.tobytes() and idx.tobytes() == wi.tobytes(), obj
        assert ri.bounds(obj).tobytes() == wb.tobytes() == ref.tree_bounds(obj).tobytes(), obj
        assert (ri.info() if obj < 0 else ri.object_info(obj))["depth"] == _depth(nodes, M)
    assert ri.bounds(0).tobytes() == ref.tree_bounds(0).tobytes()


def test_the_one_primitive_object_has_no_tree(built):
    _, ri, ref, _, _, _ = built
    assert ref.prims(1)[0].shape[0] == 1
    assert ri.object_info(1) == {"nodes": 0, "leaves": 0, "prim_refs": 0, "depth": 0}
    nodes, idx = ri.object_copy(1)
    assert nodes.shape == (0, 2) and idx.shape == (0,)


def test_info_agrees_with_the_copies(hprt, built):
    _, ri, _, _, kd, M = built
    inf = ri.info()
    assert inf["objects"] == 3 and inf["object_trees"] == 2 and inf["instances"] == 6 and inf["M"] == M and inf["kd_aware"] == int(kd)
    mask = (1 << _off(M)) - 1
    depths = []
    for obj in (-1, 0, 2):
        nodes, idx = ri.copy() if obj < 0 else ri.object_copy(obj)
        i = inf if obj < 0 else ri.object_info(obj)
        assert i["nodes"] == nodes.shape[0] and i["prim_refs"] == idx.shape[0]
        assert i["leaves"] == int(((nodes[:, 1] & mask) == M).sum()) and i["depth"] == _depth(nodes, M)
        if obj >= 0:
            depths.append(i["depth"])
    assert inf["object_depth"] == max(depths)
    assert ri.directions().shape == (M, 3)
    with pytest.raises(hprt.HprtError) as e:
        ri.object_info(3)
    assert e.value.code == hprt.E_INVALID


@pytest.mark.parametrize("kd", [False, True])
def test_the_accelerator_lines_maxdepth_reaches_every_tree(hprt, tmp_path, kd):
    """(maxdepth -1 resolves from each tree's own primitive count: the comparisons with from_triangles and Build above cover it)"""
    m, _ = rs.bake(hprt, tmp_path, rs.scene_text(kd, 7, ' "integer maxdepth" [1]'), "md1")
    ri = hprt.RbspInst(m, kd_aware=kd)
    assert ri.info()["depth"] == 1 and ri.object_info(0)["depth"] == 1 and ri.object_info(2)["depth"] == 1 and ri.info()["object_depth"] == 1
    assert ri.info()["M"] == 7


@pytest.mark.parametrize("kd", [False, True])
def test_keyword_parameters_replace_the_accelerator_line(hprt, tmp_path, kd):
    m, path = rs.bake(hprt, tmp_path, rs.scene_text(kd, 7, PARAMS), "kw")
    ri = hprt.RbspInst(m, kd_aware=kd, n_directions=9)             # nbDirections 9 and the DEFAULTS, not the line's parameters
    assert ri.info()["M"] == 9
    ref = rbspinst_ref.RbspInstScene(path, 9, kd)
    want = (hprt.RbspKd if kd else hprt.Rbsp).from_triangles(ref.prims(0)[1], n_directions=9)
    assert ri.object_copy(0)[0].tobytes() == want.arrays()[0].tobytes()
    with pytest.raises(hprt.HprtError) as e:
        hprt.RbspInst(m, kd_aware=kd, n_directions=5)
    assert e.value.code == hprt.E_UNSUPPORTED and "nbDirections" in str(e.value)


@pytest.mark.parametrize("kd", [False, True])
def test_a_model_without_instances_is_refused(hprt, tmp_path, kd):
    m, _ = rs.bake(hprt, tmp_path, rs.no_instances(kd, 7), "plain")
    with pytest.raises(hprt.HprtError) as e:
        hprt.RbspInst(m, kd_aware=kd)
    assert e.value.code == hprt.E_UNSUPPORTED and "hprt_rbsp_build" in str(e.value)
    assert (hprt.RbspKd if kd else hprt.Rbsp)(m).info()["nodes"] >= 1


@pytest.mark.parametrize("kd", [False, True])
def test_the_two_level_depth_rule(hprt, tmp_path, kd):
    """depth(top) + deepest object depth + 1 may be 64 and not 65: hand-made staircases of known depth (tests/deep_todo.py) in
    place of the built trees"""
    pair = rs.DeepPair(kd)
    m, path = rs.bake(hprt, tmp_path, pair.text(), "deep")
    ri, ref = hprt.RbspInst(m, kd_aware=kd), rbspinst_ref.RbspInstScene(path, pair.M, kd)
    pair.install(ri, ref)
    inf = ri.info()
    assert inf["depth"] == rs.TOP_LEVELS and inf["object_depth"] == rs.OBJECT_LEVELS and inf["depth"] + inf["object_depth"] + 1 == deep_todo.CAPACITY
    deeper = rs.DeepPair(kd, rs.OBJECT_LEVELS + 1)
    m2, path2 = rs.bake(hprt, tmp_path, deeper.text(), "deeper")
    ri2, ref2 = hprt.RbspInst(m2, kd_aware=kd), rbspinst_ref.RbspInstScene(path2, deeper.M, kd)
    before = ri2.object_copy(0)
    trees = deeper.trees()
    ri2.set_tree(-1, *trees[-1], ref2.tree_bounds(-1))                   # 5 levels on top: still fine over the built object tree
    with pytest.raises(hprt.HprtError) as e:
        ri2.set_tree(0, *trees[0], ref2.tree_bounds(0))                  # 5 + 59 + 1
    assert e.value.code == hprt.E_UNSUPPORTED and "maxdepth" in str(e.value)
    after = ri2.object_copy(0)
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()      # the refused tree left the handle alone
    # the rule in the restatement's own terms: every even ray of the accepted pair holds exactly the capacity
    o, d, tm = pair.deep_rays(512)
    todo = ref.intersect(o, d, tm)[5]
    assert todo.max() == deep_todo.CAPACITY and (todo[::2] == deep_todo.CAPACITY).all()
    assert (todo <= 8).any() and (todo == 9).any()                        # both sides of the walk's eight LDS entries
    assert ref.occluded(o, d, tm)[2].max() <= deep_todo.CAPACITY


def test_the_existing_rbsp_entry_points_and_warnings_are_unchanged(hprt, built):
    m, _, _, _, kd, M = built
    name = "rbspkd" if kd else "rbsp"
    assert m.accelerator == name
    w = m.warnings()
    assert 'Accelerator "%s" is outside the hot-path scope; "bvh" used' % name in w, w
    assert not any("rbspinst" in x for x in w), w
    with pytest.raises(hprt.HprtError) as e:
        (hprt.RbspKd if kd else hprt.Rbsp)(m)
    assert e.value.code == hprt.E_UNSUPPORTED and "trees over object instances are not supported" in str(e.value)
    hprt.Bvh(m)
