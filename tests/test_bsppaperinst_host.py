"""Two-level general BSP trees on the host (hprt_bsppaperinst_*): what the already pinned general BSP builder is FED — every object's
primitives in object space, the top level's with an instance as a non-triangle bounded by TransformedPrimitive::WorldBound and so
without planes of its own, the parameters of the Accelerator line per tree — the handle's info and copies, the refusals, the depth
rule, and that the existing bsppaper / bsppaperkd entry points and warnings stay as they are.  (The attaches' refusals need a scene
on a device: tests/test_gpu_bsppaperinst.py.)"""
import ctypes as C

import numpy as np
import pytest

import bsppaperinst_ref
import bsppaperinst_scenes as bs
import deep_todo

PARAMS = ' "integer maxprims" [2] "float emptybonus" [0.2] "integer intersectcost" [40] "integer traversalcost" [3]'
KW = dict(max_prims=2, empty_bonus=0.2, isect_cost=40, trav_cost=3)


def layout(kd):
    """(shift, mask, leaf tag) of BSPNode's / BSPKdNode's flags"""
    return (3, 7, 3) if kd else (1, 1, 1)


@pytest.fixture(scope="module", params=[(kd, p) for kd in (False, True) for p in ("defaults", "parameters")],
                ids=lambda c: "%s-%s" % ("bsppaperkd" if c[0] else "bsppaper", c[1]))
def built(request, hprt, tmp_path_factory):
    kd, which = request.param
    with_params = which == "parameters"
    m, path = bs.bake(hprt, tmp_path_factory.mktemp("bsppaperinst"), bs.scene_text(kd, PARAMS if with_params else ""), "scene")
    return m, hprt.BspPaperInst(m, kd_aware=kd), bsppaperinst_ref.BspPaperInstScene(path, kd), (KW if with_params else {}), kd


def _depth(nodes, kd):
    """interior levels of the deepest path"""
    off, mask, leaf = layout(kd)

    def rec(k):
        if nodes[k, 1] & mask == leaf:
            return 0
        return 1 + max(rec(k + 1), rec(int(nodes[k, 1] >> off)))
    return rec(0)


def _interior(nodes, kd):
    """(kd or axis-sweep interior nodes, plane interior nodes) as the info words count them: kd-aware by the flags, plain by
    whether the axis is a coordinate axis"""
    off, mask, leaf = layout(kd)
    kind = nodes[:, 1] & mask
    inner = kind != leaf
    if kd:
        return int((inner & (kind < 3)).sum()), int((kind == 4).sum())
    axes = nodes[:, 2:5].copy().view(np.float32)
    one = (axes != 0).sum(axis=1) == 1
    return int((inner & one).sum()), int((inner & ~one).sum())


def _lib_planes(hprt, tri9):
    fn = hprt.lib.hprt_debug_bsppaper_planes
    fn.restype = C.c_int
    tri9 = np.ascontiguousarray(tri9, np.float32).reshape(9)
    out = np.zeros((4, 4), np.float32); k = C.c_uint32()
    assert fn(tri9.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.byref(k)) == 0
    return out[:k.value]


def test_the_triangle_objects_tree_is_the_pinned_builders_over_its_object_space_triangles(hprt, built):
    m, bi, ref, kw, kd = built
    tri, p9, lo, hi = ref.prims(bs.BLOB)
    assert tri.all() and p9.shape == (20, 9) and p9.tobytes() == bs.blob_triangles().tobytes()
    want = (hprt.BspPaperKd if kd else hprt.BspPaper).from_triangles(p9, **kw)
    nodes, idx = bi.object_copy(bs.BLOB)
    wn, wi = want.arrays()
    assert nodes.shape[1] == 5 and nodes.tobytes() == wn.tobytes() and idx.tobytes() == wi.tobytes()      # nodes, axes, primitiveIndices
    assert bi.object_info(bs.BLOB)["depth"] == want.info()["depth"] and bi.object_info(bs.BLOB)["leaves"] == want.info()["leaves"]


def test_the_top_level_and_the_mixed_objects_trees_are_the_restated_builds_over_the_restatements_lists(built):
    m, bi, ref, kw, kd = built
    assert (ref.n_top, ref.n_objects, ref.n_instances) == (bs.N_TOP, bs.N_OBJECTS, bs.N_INSTANCES)
    tri, _, _, _ = ref.prims(-1)
    assert tri.tolist() == [1, 1, 0] + [0] * bs.N_INSTANCES        # floor triangles, the sphere, the instances
    tri, p9, _, _ = ref.prims(bs.MIX)
    assert tri.tolist() == [0, 1, 1] and not p9[0].any()             # the sphere has no vertices
    for obj in (-1, bs.MIX):
        wn, wi, wb = ref.build(obj, **kw)
        nodes, idx = bi.copy() if obj < 0 else bi.object_copy(obj)
        assert nodes.tobytes() == wn.tobytes() and idx.tobytes() == wi.tobytes(), obj
        assert bi.bounds(obj).tobytes() == wb.tobytes() == ref.tree_bounds(obj).tobytes(), obj
        assert (bi.info() if obj < 0 else bi.object_info(obj))["depth"] == _depth(nodes, kd)
    assert bi.bounds(bs.BLOB).tobytes() == ref.tree_bounds(bs.BLOB).tobytes()


@pytest.mark.parametrize("kd", [False, True])
def test_the_top_levels_oblique_planes_are_its_triangles_own(hprt, tmp_path, kd):
    """An instance is a TransformedPrimitive: no planes of its own.  Every plane of the top-level tree that is not an axis plane
    is therefore one of getBSPPaperPlanes of a top-level TRIANGLE — and under the default parameters there are such planes (the
    floor's diagonal), or this would test nothing."""
    m, path = bs.bake(hprt, tmp_path, bs.scene_text(kd), "oblique")
    bi, ref = hprt.BspPaperInst(m, kd_aware=kd), bsppaperinst_ref.BspPaperInstScene(path, kd)
    off, mask, leaf = layout(kd)
    nodes, _ = bi.copy()
    axes = nodes[:, 2:5].copy().view(np.float32)
    split = nodes[:, 0].copy().view(np.float32)
    kind = nodes[:, 1] & mask
    oblique = (kind != leaf) & ((axes != 0).sum(axis=1) > 1)
    assert oblique.any()
    tri, p9, _, _ = ref.prims(-1)
    planes = np.concatenate([_lib_planes(hprt, p9[i]) for i in np.nonzero(tri)[0]])
    have = {p.tobytes() for p in planes}
    for k in np.nonzero(oblique)[0]:
        assert np.array([split[k], *axes[k]], np.float32).tobytes() in have, k


def test_kd_aware_trees_hold_kd_and_plane_nodes_on_both_levels(hprt, tmp_path):
    m, _ = bs.bake(hprt, tmp_path, bs.scene_text(True), "kdaware")
    bi = hprt.BspPaperInst(m, kd_aware=True)
    for nodes in (bi.copy()[0], bi.object_copy(bs.BLOB)[0]):
        n_kd, n_plane = _interior(nodes, True)
        assert n_kd > 0 and n_plane > 0
        axes = nodes[:, 2:5].copy().view(np.float32)
        assert not axes[(nodes[:, 1] & 7) != 4].any()                # kd nodes and leaves carry no axis


def test_the_one_primitive_objects_have_no_tree(built):
    _, bi, ref, _, _ = built
    for obj in (bs.ONE, bs.LAST):
        assert ref.prims(obj)[0].shape[0] == 1
        assert bi.object_info(obj) == {"nodes": 0, "leaves": 0, "prim_refs": 0, "depth": 0}
        nodes, idx = bi.object_copy(obj)
        assert nodes.shape == (0, 5) and idx.shape == (0,)
    assert bs.LAST == ref.n_objects - 1                              # the last object defined: its leaf ends the attached node array


def test_info_agrees_with_the_copies(hprt, built):
    _, bi, _, _, kd = built
    inf = bi.info()
    assert inf["objects"] == bs.N_OBJECTS and inf["object_trees"] == 2 and inf["instances"] == bs.N_INSTANCES
    assert inf["kd_aware"] == int(kd) and inf["reserved"] == 0
    off, mask, leaf = layout(kd)
    depths, n_axis, n_plane = [], 0, 0
    for obj in (-1, bs.BLOB, bs.MIX):
        nodes, idx = bi.copy() if obj < 0 else bi.object_copy(obj)
        i = inf if obj < 0 else bi.object_info(obj)
        assert i["nodes"] == nodes.shape[0] and i["prim_refs"] == idx.shape[0]
        assert i["leaves"] == int(((nodes[:, 1] & mask) == leaf).sum()) and i["depth"] == _depth(nodes, kd)
        a, p = _interior(nodes, kd)
        n_axis += a; n_plane += p
        assert a + p + i["leaves"] == i["nodes"]
        if obj >= 0:
            depths.append(i["depth"])
    assert inf["object_depth"] == max(depths)
    assert (inf["axis_interior"], inf["plane_interior"]) == (n_axis, n_plane)
    with pytest.raises(hprt.HprtError) as e:
        bi.object_info(bs.N_OBJECTS)
    assert e.value.code == hprt.E_INVALID


@pytest.mark.parametrize("kd", [False, True])
def test_the_accelerator_lines_maxdepth_reaches_every_tree(hprt, tmp_path, kd):
    """(maxdepth -1 resolves from each tree's own primitive count: the comparisons with from_triangles and Build above cover it)"""
    m, _ = bs.bake(hprt, tmp_path, bs.scene_text(kd, ' "integer maxdepth" [1]'), "md1")
    bi = hprt.BspPaperInst(m, kd_aware=kd)
    assert bi.info()["depth"] == 1 and bi.object_info(bs.BLOB)["depth"] == 1 and bi.object_info(bs.MIX)["depth"] == 1 and bi.info()["object_depth"] == 1


@pytest.mark.parametrize("kd", [False, True])
def test_keyword_parameters_replace_the_accelerator_line(hprt, tmp_path, kd):
    m, path = bs.bake(hprt, tmp_path, bs.scene_text(kd, PARAMS), "kw")
    bi = hprt.BspPaperInst(m, kd_aware=kd, isect_cost=80)           # isect_cost given: the DEFAULTS otherwise, not the line's parameters
    ref = bsppaperinst_ref.BspPaperInstScene(path, kd)
    cls = hprt.BspPaperKd if kd else hprt.BspPaper
    p9 = ref.prims(bs.BLOB)[1]
    assert bi.object_copy(bs.BLOB)[0].tobytes() == cls.from_triangles(p9).arrays()[0].tobytes()
    line = hprt.BspPaperInst(m, kd_aware=kd)
    assert line.object_copy(bs.BLOB)[0].tobytes() == cls.from_triangles(p9, **KW).arrays()[0].tobytes()
    assert line.object_copy(bs.BLOB)[0].tobytes() != bi.object_copy(bs.BLOB)[0].tobytes()
    deep = hprt.BspPaperInst(m, kd_aware=kd, isect_cost=80, max_depth=2)
    assert deep.info()["depth"] <= 2 and deep.info()["object_depth"] == 2


@pytest.mark.parametrize("kd", [False, True])
def test_a_model_without_instances_is_refused(hprt, tmp_path, kd):
    m, _ = bs.bake(hprt, tmp_path, bs.no_instances(kd), "plain")
    with pytest.raises(hprt.HprtError) as e:
        hprt.BspPaperInst(m, kd_aware=kd)
    assert e.value.code == hprt.E_UNSUPPORTED and "hprt_bsppaper_build" in str(e.value)
    assert (hprt.BspPaperKd if kd else hprt.BspPaper)(m).info()["nodes"] >= 1


@pytest.mark.parametrize("kd", [False, True])
def test_the_two_level_depth_rule(hprt, tmp_path, kd):
    """depth(top) + deepest object depth + 1 may be 64 and not 65: hand-made staircases of known depth (tests/deep_todo.py) in
    place of the built trees"""
    pair = bs.DeepPair(kd)
    m, path = bs.bake(hprt, tmp_path, pair.text(), "deep")
    bi, ref = hprt.BspPaperInst(m, kd_aware=kd), bsppaperinst_ref.BspPaperInstScene(path, kd)
    pair.install(bi, ref)
    inf = bi.info()
    assert inf["depth"] == bs.TOP_LEVELS and inf["object_depth"] == bs.OBJECT_LEVELS and inf["depth"] + inf["object_depth"] + 1 == deep_todo.CAPACITY
    for obj, (nodes, idx) in pair.trees().items():                   # copy() returns what set_tree took
        got = bi.copy() if obj < 0 else bi.object_copy(obj)
        assert got[0].tobytes() == nodes.tobytes() and got[1].tobytes() == idx.tobytes()
    deeper = bs.DeepPair(kd, bs.OBJECT_LEVELS + 1)
    m2, path2 = bs.bake(hprt, tmp_path, deeper.text(), "deeper")
    bi2, ref2 = hprt.BspPaperInst(m2, kd_aware=kd), bsppaperinst_ref.BspPaperInstScene(path2, kd)
    before = bi2.object_copy(0)
    trees = deeper.trees()
    bi2.set_tree(-1, *trees[-1], ref2.tree_bounds(-1))                   # 5 levels on top: still fine over the built object tree
    with pytest.raises(hprt.HprtError) as e:
        bi2.set_tree(0, *trees[0], ref2.tree_bounds(0))                  # 5 + 59 + 1
    assert e.value.code == hprt.E_UNSUPPORTED and "maxdepth" in str(e.value)
    after = bi2.object_copy(0)
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()      # the refused tree left the handle alone
    # the rule in the restatement's own terms: every even ray of the accepted pair holds exactly the capacity
    o, d, tm = pair.deep_rays(512)
    todo = ref.intersect(o, d, tm)[5]
    assert todo.max() == deep_todo.CAPACITY and (todo[::2] == deep_todo.CAPACITY).all()
    assert (todo <= 8).any() and (todo == 9).any()                        # both sides of the walk's eight LDS entries
    assert ref.occluded(o, d, tm)[2].max() <= deep_todo.CAPACITY


def test_set_tree_refuses_a_zero_axis_at_a_plane_node(hprt, built):
    _, bi, ref, _, kd = built
    off, mask, leaf = layout(kd)
    nodes, idx = bi.object_copy(bs.BLOB)
    kind = nodes[:, 1] & mask
    plane = np.nonzero(kind == 4 if kd else kind != leaf)[0]
    assert plane.size
    bad = nodes.copy()
    bad[plane[0], 2:5] = 0
    with pytest.raises(hprt.HprtError) as e:
        bi.set_tree(bs.BLOB, bad, idx, ref.tree_bounds(bs.BLOB))
    assert e.value.code == hprt.E_INVALID and "malformed tree" in str(e.value)
    after = bi.object_copy(bs.BLOB)
    assert after[0].tobytes() == nodes.tobytes() and after[1].tobytes() == idx.tobytes()
    bi.set_tree(bs.BLOB, nodes, idx, ref.tree_bounds(bs.BLOB))          # and its own copy is taken back
    assert bi.object_copy(bs.BLOB)[0].tobytes() == nodes.tobytes()
    with pytest.raises(hprt.HprtError) as e:
        bi.set_tree(bs.LAST, nodes, idx, ref.tree_bounds(bs.BLOB))
    assert e.value.code == hprt.E_INVALID and "one primitive" in str(e.value)


def test_the_existing_bsppaper_entry_points_and_warnings_are_unchanged(hprt, built):
    m, _, _, _, kd = built
    name = "bsppaperkd" if kd else "bsppaper"
    assert m.accelerator == name
    w = m.warnings()
    assert any('"%s" is outside the hot-path scope; "bvh" used' % name in x for x in w), w
    assert not any("bsppaperinst" in x for x in w) and not any("hprt_scene_attach_" + name in x for x in w), w
    with pytest.raises(hprt.HprtError) as e:
        (hprt.BspPaperKd if kd else hprt.BspPaper)(m)
    assert e.value.code == hprt.E_UNSUPPORTED and "%s trees over object instances are not supported (the scene keeps its BVH)" % name in str(e.value)
    hprt.Bvh(m)
