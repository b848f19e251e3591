"""Two-level kd-trees on the host (hprt_kdinst_*): what the already pinned kd-tree builder is FED — every object's primitive
bounds in object space, the top level's with TransformedPrimitive::WorldBound for the instances, the parameters of the Accelerator
line per tree — the handle's info and copies, the refusals, and that the existing kd entry points and warnings stay as they are."""
import numpy as np
import pytest

import deep_todo
import kdinst_ref
import kdinst_scenes as ks

PARAMS = ' "integer maxprims" [2] "float emptybonus" [0.2] "integer intersectcost" [40] "integer traversalcost" [3]'
KW = dict(max_prims=2, empty_bonus=0.2, isect_cost=40, trav_cost=3)


@pytest.fixture(scope="module", params=["defaults", "parameters"])
def built(request, hprt, tmp_path_factory):
    with_params = request.param == "parameters"
    m, path = ks.bake(hprt, tmp_path_factory.mktemp("kdinst"), ks.scene_text(PARAMS if with_params else ""), "scene")
    return m, hprt.KdInst(m), kdinst_ref.KdInstScene(path), (KW if with_params else {})


def _depth(nodes):
    """interior levels of the deepest path"""
    def rec(k):
        if nodes[k, 1] & 3 == 3:
            return 0
        return 1 + max(rec(k + 1), rec(int(nodes[k, 1] >> 2)))
    return rec(0)


def test_every_tree_is_the_pinned_builders_over_the_right_bounds(hprt, built):
    m, kd, ref, kw = built
    assert (ref.n_top, ref.n_objects, ref.n_instances) == (2 + 1 + 6, 3, 6)
    for obj in (-1, 0, 2):
        lo, hi = ref.prim_bounds(obj)
        assert lo.shape[0] == {-1: 9, 0: 20, 2: 3}[obj]
        want = hprt.KdTree.from_bounds(lo, hi, **kw)
        nodes, idx = kd.copy() if obj < 0 else kd.object_copy(obj)
        wn, wi = want.arrays()
        assert nodes.tobytes() == wn.tobytes() and idx.tobytes() == wi.tobytes(), obj
        assert (kd.info() if obj < 0 else kd.object_info(obj))["depth"] == want.info()["depth"]
        assert kd.bounds(obj).tobytes() == ref.tree_bounds(obj).tobytes(), obj


def test_the_accelerator_lines_maxdepth_reaches_every_tree(hprt, tmp_path):
    """(maxdepth -1 resolves from each tree's own primitive count: the comparison with from_bounds above covers it)"""
    m, _ = ks.bake(hprt, tmp_path, ks.scene_text(' "integer maxdepth" [1]'), "md1")
    kd = hprt.KdInst(m)
    assert kd.info()["depth"] == 1 and kd.object_info(0)["depth"] == 1 and kd.object_info(2)["depth"] == 1 and kd.info()["object_depth"] == 1


def test_the_one_primitive_object_has_no_tree(built):
    _, kd, ref, _ = built
    assert ref.prim_bounds(1)[0].shape[0] == 1
    assert kd.object_info(1) == {"nodes": 0, "leaves": 0, "prim_refs": 0, "depth": 0}
    nodes, idx = kd.object_copy(1)
    assert nodes.shape == (0, 2) and idx.shape == (0,)


def test_info_agrees_with_the_copies(hprt, built):
    _, kd, _, _ = built
    inf = kd.info()
    assert inf["objects"] == 3 and inf["object_trees"] == 2 and inf["instances"] == 6
    depths = []
    for obj in (-1, 0, 2):
        nodes, idx = kd.copy() if obj < 0 else kd.object_copy(obj)
        i = inf if obj < 0 else kd.object_info(obj)
        assert i["nodes"] == nodes.shape[0] and i["prim_refs"] == idx.shape[0]
        assert i["leaves"] == int(((nodes[:, 1] & 3) == 3).sum()) and i["depth"] == _depth(nodes)
        if obj >= 0:
            depths.append(i["depth"])
    assert inf["object_depth"] == max(depths)
    with pytest.raises(hprt.HprtError) as e:
        kd.object_info(3)
    assert e.value.code == hprt.E_INVALID


def test_a_model_without_instances_is_refused(hprt, tmp_path):
    m, _ = ks.bake(hprt, tmp_path, ks.NO_INSTANCES, "plain")
    with pytest.raises(hprt.HprtError) as e:
        hprt.KdInst(m)
    assert e.value.code == hprt.E_UNSUPPORTED and "hprt_kdtree_build" in str(e.value)
    assert hprt.KdTree(m).info()["nodes"] >= 1


def test_the_two_level_depth_rule(hprt, tmp_path):
    """depth(top) + deepest object depth + 1 may be 64 and not 65: hand-made staircases of known depth (tests/deep_todo.py) in
    place of the built trees"""
    pair = ks.DeepPair()
    m, path = ks.bake(hprt, tmp_path, pair.text(), "deep")
    kd, ref = hprt.KdInst(m), kdinst_ref.KdInstScene(path)
    pair.install(kd, ref)
    inf = kd.info()
    assert inf["depth"] == ks.TOP_LEVELS and inf["object_depth"] == ks.OBJECT_LEVELS and inf["depth"] + inf["object_depth"] + 1 == deep_todo.CAPACITY
    deeper = ks.DeepPair(ks.OBJECT_LEVELS + 1)
    m2, path2 = ks.bake(hprt, tmp_path, deeper.text(), "deeper")
    kd2, ref2 = hprt.KdInst(m2), kdinst_ref.KdInstScene(path2)
    before = kd2.object_copy(0)
    nodes, idx = deeper.top.kdtree()
    kd2.set_tree(-1, nodes, idx, ref2.tree_bounds(-1))                   # 5 levels on top: still fine over the built object tree
    nodes, idx = deeper.obj.kdtree()
    with pytest.raises(hprt.HprtError) as e:
        kd2.set_tree(0, nodes, idx, ref2.tree_bounds(0))                 # 5 + 59 + 1
    assert e.value.code == hprt.E_UNSUPPORTED and "maxdepth" in str(e.value)
    after = kd2.object_copy(0)
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()      # the refused tree left the handle alone
    # the rule in the restatement's own terms: the deepest ray of the accepted pair holds exactly the capacity
    o, d, tm = pair.deep_rays(512)
    todo = ref.intersect(o, d, tm)[5]
    assert todo.max() == deep_todo.CAPACITY and (todo[::2] == deep_todo.CAPACITY).all()
    assert (todo <= 8).any() and (todo == 9).any()                        # both sides of the walk's eight LDS entries
    assert ref.occluded(o, d, tm)[2].max() <= deep_todo.CAPACITY


def test_the_built_pair_of_a_deep_point_cloud_is_refused(hprt, tmp_path):
    """the same rule through the builder: an object of 100,000 points with a full empty bonus goes 73 levels deep when "integer
    maxdepth" lets it (tests/test_kdtree_fallbacks.py) and is refused; with maxdepth 20 the pair is built"""
    rng = np.random.default_rng(1)
    P = np.repeat(rng.uniform(0, 1, (100000, 3)).astype(np.float32), 3, 0)
    mesh = 'Shape "trianglemesh" "integer indices" [%s] "point P" [%s]\n' % (" ".join(map(str, range(P.shape[0]))), " ".join("%.5f" % v for v in P.ravel()))
    text = (ks.HEAD % ' "integer maxdepth" [%d] "float emptybonus" [1.0]' + 'ObjectBegin "cloud"\n' + mesh + "ObjectEnd\n" +
            ks.FLOOR + ks._inst("cloud", "Translate 0 0 1") + ks._inst("cloud", "Translate 2 0 1") + "WorldEnd\n")
    m, _ = ks.bake(hprt, tmp_path, text % 300, "cloud300")
    with pytest.raises(hprt.HprtError) as e:
        hprt.KdInst(m)
    assert e.value.code == hprt.E_UNSUPPORTED and "maxdepth" in str(e.value)
    m20, _ = ks.bake(hprt, tmp_path, text % 20, "cloud20")
    d = hprt.KdInst(m20).info()
    assert d["object_depth"] == 20 and d["depth"] + d["object_depth"] + 1 <= 64


def test_the_existing_kd_entry_points_and_warnings_are_unchanged(hprt, built):
    m, _, _, _ = built
    assert m.accelerator == "kdtree"
    w = m.warnings()
    assert 'Accelerator "kdtree" is outside the hot-path scope; "bvh" used' in w, w
    assert not any("kdinst" in x for x in w), w
    with pytest.raises(hprt.HprtError) as e:
        hprt.KdTree(m)
    assert e.value.code == hprt.E_UNSUPPORTED and "kd-trees over object instances are not supported" in str(e.value)
    hprt.Bvh(m)
