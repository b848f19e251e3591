"""Two-level node-based BSP trees on the host (hprt_bspnodeinst_build, hprt.BspNodeInst): what the already pinned node-based builder
is FED on the two levels of an instanced scene — every object's primitives in object space, the top level's with an instance as a
primitive with a zero normal and its world bound — for the nine accelerator names; every tree from a fresh std::mt19937(seed);
degenerate top levels made only or mostly of instances; the handle's info words; the refusals in their order; the tie-free seeds of
tests/bspnodeinst_fuzz.py; and that the single-level entries, their messages and the front end's warning stay as they are.  The
restated builds are tests/bspnodeinst_reference.cpp's, the restated walk tests/bsppaperinst_reference.cpp's over the library's trees.
(Fails on the parent, where hprt.BspNodeInst does not exist.  The attaches' refusals need a device: tests/test_gpu_bspnodeinst.py.)

Two refusals of the entry's list cannot be provoked through it and are held where they can be.  A tree's own refusal (a drawn index
equal to the primitive count, fastkd's undefined case, the reference's primitive buffer outgrown) needs inputs nobody has found for
the single-level builds either; the prefix "object N:" / "top level:" is BuildTwoLevel's, shared with the other two-level handles.
No build of a small scene reaches 64 levels over both trees; the depth rule is the handle's existing overload, held here through
set_tree on a BspNodeInst handle, plain and kd-aware."""
import ctypes as C

import numpy as np
import pytest

import bspnode_ref
import bspnodeinst_fuzz as nf
import bspnodeinst_ref as nr
import bspnodeinst_scenes as ns
import bsppaperinst_ref
import deep_todo
import tree_fuzz as tf
from test_gpu_fuzz import random_scene
from tree_walk_checks import _bits

ACCS = ns.ACCELERATORS
KS, SEEDS = (4, 6), (5489, 7)


def _params(hprt, accelerator, K, seed=5489, **kw):
    chooser, form = bspnode_ref.split(accelerator)
    d = dict(isect_cost=80, trav_cost=5, kd_trav_cost=1, empty_bonus=0.0, max_prims=1, max_depth=-1, threads=0)
    d.update(kw)
    return hprt.BspNodeParams(chooser, form, K, seed, d["isect_cost"], d["trav_cost"], d["kd_trav_cost"], d["empty_bonus"], d["max_prims"], d["max_depth"],
                              d["threads"])


@pytest.fixture(scope="module")
def own(hprt, tmp_path_factory):
    """(model, restated build) of the own scene; the Accelerator line names one of the nine, the tests pass theirs"""
    m, path = ns.bake(hprt, tmp_path_factory.mktemp("bspnodeinst"), ns.scene_text("bspcluster"), "scene")
    return m, nr.BspNodeInstBuild(path), path


@pytest.fixture(scope="module")
def simple(hprt):
    return hprt.Model.load(ns.SIMPLE_INSTANCED), nr.BspNodeInstBuild(ns.SIMPLE_INSTANCED), ns.SIMPLE_INSTANCED


def test_what_the_restatement_feeds_its_builds(own, simple):
    _, ref, _ = own
    assert (ref.n_top, ref.n_objects, ref.n_instances) == (ns.N_TOP, ns.N_OBJECTS, ns.N_INSTANCES)
    tri, p9, lo, hi = ref.prims(-1)
    assert tri.tolist() == [1, 1, 0] + [0] * ns.N_INSTANCES              # floor triangles, the sphere, the instances
    assert not p9[2:].any() and (hi[3:] > lo[3:]).all()                   # an instance: no vertices (a zero normal), its world bound
    assert ref.tree_objects() == [ns.BLOB, ns.MIX]
    _, sref, _ = simple
    assert (sref.n_top, sref.n_instances) == (1, 1) and sref.prims(-1)[0].tolist() == [0]      # a top level of one instance


@pytest.mark.parametrize("acc", ACCS)
@pytest.mark.parametrize("which", ["own", "simple"])
def test_every_tree_is_the_restated_build(hprt, own, simple, which, acc):
    m, ref, _ = own if which == "own" else simple
    for K in KS:
        for seed in SEEDS:
            t = hprt.BspNodeInst(m, acc, n_directions=K, seed=seed)
            nr.assert_same_trees(t, ref, acc, n_directions=K, seed=seed)
            assert t.info()["kd_aware"] == int(nr.fastkd(acc)) and t.build_stats is None


@pytest.mark.parametrize("acc", ACCS)
def test_the_triangle_objects_tree_is_the_single_level_builders_with_the_same_seed(hprt, own, acc):
    """every tree starts a fresh std::mt19937(seed): the object's tree does not depend on what was built before it"""
    m, ref, _ = own
    tri, p9, _, _ = ref.prims(ns.BLOB)
    assert tri.all() and p9.shape == (20, 9)
    cls = hprt.BspNodeKd if nr.fastkd(acc) else hprt.BspNode
    for K in KS:
        for seed in SEEDS:
            want = cls.from_triangles(p9, acc, n_directions=K, seed=seed)
            bi = hprt.BspNodeInst(m, acc, n_directions=K, seed=seed)
            nodes, idx = bi.object_copy(ns.BLOB)
            wn, wi = want.arrays()
            assert nodes.tobytes() == wn.tobytes() and idx.tobytes() == wi.tobytes()
            assert bi.object_info(ns.BLOB)["depth"] == want.info()["depth"] and bi.object_info(ns.BLOB)["leaves"] == want.info()["leaves"]


@pytest.mark.parametrize("acc", ACCS)
@pytest.mark.parametrize("lone", [False, True], ids=["only-instances", "one-triangle-beside"])
def test_degenerate_top_levels(hprt, tmp_path, lone, acc):
    """A top level of three instances (and one with a lone triangle in front): all or all but one of the normals the choosers see
    are zero.  chooseArbitraryNormals hands out zero vectors, which have no candidate; calculateClusterMeans returns the zero
    normals as they are for np <= K and otherwise clusters them at Angle = acos(0), redraws the means of empty clusters 500 times
    over, and for one cluster normalises a zero sum to NaN.  The library does what the restatement does, byte for byte — or both
    refuse."""
    m, path = ns.bake(hprt, tmp_path, ns.only_instances_text(acc, lone), "degenerate")
    ref = nr.BspNodeInstBuild(path)
    n_top = 3 + int(lone)
    assert ref.n_top == n_top and ref.prims(-1)[0].tolist() == ([1] if lone else []) + [0, 0, 0] and ref.tree_objects() == [0]
    plain = not (acc.endswith("withkd") or acc.endswith("fastkd"))
    built = 0
    for K in ((1, 2, 3, 5) if plain else (3, 4, 5, 8)):          # chosen directions: fewer than, as many as and more than the primitives
        for seed in SEEDS:
            try:
                want = [ref.build(obj, acc, n_directions=K, seed=seed) for obj in (-1, 0)]
            except RuntimeError:
                with pytest.raises(hprt.HprtError) as e:
                    hprt.BspNodeInst(m, acc, n_directions=K, seed=seed)
                assert e.value.code == hprt.E_UNSUPPORTED
                continue
            t = hprt.BspNodeInst(m, acc, n_directions=K, seed=seed)
            nr.assert_same_trees(t, ref, acc, n_directions=K, seed=seed)
            assert t.info()["nodes"] == want[0][0].shape[0] >= 1
            built += 1
    assert built > 0


def test_the_tree_does_not_depend_on_the_thread_count(hprt, own):
    m, _, _ = own
    for acc in ("bspclusterfastkd", "bsprandomwithkd", "bsparbitrary"):
        a, b = (hprt.BspNodeInst(m, acc, n_directions=6, seed=7, threads=n) for n in (1, 7))
        for obj in (-1, ns.BLOB, ns.MIX):
            ta, tb = (t.copy() if obj < 0 else t.object_copy(obj) for t in (a, b))
            assert ta[0].tobytes() == tb[0].tobytes() and ta[1].tobytes() == tb[1].tobytes()


@pytest.mark.parametrize("acc", ACCS)
def test_info_agrees_with_the_copies(hprt, own, acc):
    m, _, _ = own
    fast, withkd = nr.fastkd(acc), acc.endswith("withkd")
    bi = hprt.BspNodeInst(m, acc, n_directions=5, seed=7)
    inf = bi.info()
    assert inf["objects"] == ns.N_OBJECTS and inf["object_trees"] == 2 and inf["instances"] == ns.N_INSTANCES
    assert inf["kd_aware"] == int(fast) and inf["reserved"] == 0
    off, mask, leaf = (3, 7, 3) if fast else (1, 1, 1)
    depths, n_kd, n_plane, n_unit, n_interior = [], 0, 0, 0, 0
    for obj in (-1, ns.BLOB, ns.MIX):
        nodes, idx = bi.copy() if obj < 0 else bi.object_copy(obj)
        i = inf if obj < 0 else bi.object_info(obj)
        kind = nodes[:, 1] & mask
        assert i["nodes"] == nodes.shape[0] and i["prim_refs"] == idx.shape[0] and i["leaves"] == int((kind == leaf).sum())
        interior, unit = bspnode_ref.interior_axes(nodes, fast)
        n_interior += int(interior.sum()); n_unit += int(unit.sum())
        if fast:
            n_kd += int((kind < 3).sum()); n_plane += int((kind == 4).sum())
            axes = nodes[:, 2:5].copy().view(np.float32)
            assert not axes[kind != 4].any()                             # kd nodes and leaves carry no axis
        if obj >= 0:
            depths.append(i["depth"])
    assert inf["object_depth"] == max(depths)
    assert inf["axis_interior"] + inf["plane_interior"] == n_interior
    if fast:
        assert (inf["axis_interior"], inf["plane_interior"]) == (n_kd, n_plane) and n_kd > 0
    elif withkd:     # the axis sweep's winners are plane nodes with a unit axis; a chosen direction may be a unit axis too
        assert 0 < inf["axis_interior"] <= n_unit
    else:
        assert inf["axis_interior"] == 0
    for obj in (ns.ONE, ns.LAST):
        assert bi.object_info(obj) == {"nodes": 0, "leaves": 0, "prim_refs": 0, "depth": 0}
        assert bi.object_copy(obj)[0].shape == (0, 5)
    with pytest.raises(hprt.HprtError) as e:
        bi.object_info(ns.N_OBJECTS)
    assert e.value.code == hprt.E_INVALID


def test_the_accelerator_line_and_keywords(hprt, tmp_path):
    line = ' "integer nbDirections" [6] "integer seed" [77] "integer maxprims" [2] "integer intersectcost" [20] "integer traversalcost" [2] "float emptybonus" [0.5] "integer kdtraversalcost" [4]'
    kw = dict(n_directions=6, seed=77, max_prims=2, isect_cost=20, trav_cost=2, empty_bonus=0.5, kd_trav_cost=4)
    m, path = ns.bake(hprt, tmp_path, ns.scene_text("bsprandomfastkd", line), "line")
    ref = nr.BspNodeInstBuild(path)
    nr.assert_same_trees(hprt.BspNodeInst(m), ref, "bsprandomfastkd", **kw)                  # params NULL: the line's name and parameters
    nr.assert_same_trees(hprt.BspNodeInst(m, "bspclusterwithkd"), ref, "bspclusterwithkd")    # a name given: the keywords' defaults, not the line's
    md, _ = ns.bake(hprt, tmp_path, ns.scene_text("bspcluster", ' "integer maxdepth" [1]'), "md1")
    bi = hprt.BspNodeInst(md)
    assert bi.info()["depth"] == 1 and bi.info()["object_depth"] == 1 and bi.object_info(ns.MIX)["depth"] == 1


def test_refusals_in_their_order(hprt, own, simple, tmp_path):
    m, _, _ = own
    fn = hprt.lib.hprt_bspnodeinst_build
    bad = _params(hprt, "bspclusterwithkd", 2)          # K - 3 wraps in the reference
    good = _params(hprt, "bspclusterwithkd", 4)
    err = lambda: hprt.lib.hprt_last_error().decode()
    # 1. a null argument, whatever else is wrong
    h = C.c_void_p(0xdead)
    assert fn(None, C.byref(bad), C.byref(h)) == hprt.E_INVALID and h.value is None and "hprt_bspnodeinst_build: null argument" in err()
    assert fn(m._h, C.byref(good), None) == hprt.E_INVALID
    # 2. a model without instances, before its parameters are looked at
    flat, _ = ns.bake(hprt, tmp_path, ns.no_instances("bspcluster"), "flat")
    h = C.c_void_p(0xdead)
    assert fn(flat._h, C.byref(bad), C.byref(h)) == hprt.E_UNSUPPORTED and h.value is None
    assert "no object instances" in err() and "hprt_bspnode_build / hprt_bspnodekd_build" in err()
    assert hprt.BspNode(flat).info()["nodes"] >= 1
    # (params NULL on a model whose Accelerator line names no node-based tree: hprt_bspnode_build's wording)
    baked, _, _ = simple
    h = C.c_void_p(0xdead)
    assert fn(baked._h, None, C.byref(h)) == hprt.E_INVALID and h.value is None
    assert 'the scene\'s Accelerator "bvh" is no node-based BSP tree; pass params' in err()
    # 3. what the builder refuses from the parameters alone: no tree's prefix, the single-level entry's message
    p9 = np.zeros((1, 9), np.float32)
    for acc, K in (("bspclusterwithkd", 2), ("bsprandomfastkd", 0), ("bspcluster", 0), ("bsparbitrary", 5000)):
        q = _params(hprt, acc, K)
        h1 = C.c_void_p(0xdead)
        single = hprt.lib.hprt_bspnodekd_build_from_triangles if nr.fastkd(acc) else hprt.lib.hprt_bspnode_build_from_triangles
        assert single(1, p9.ctypes.data_as(C.c_void_p), C.byref(q), C.byref(h1)) == hprt.E_UNSUPPORTED
        said = err()
        h = C.c_void_p(0xdead)
        assert fn(m._h, C.byref(q), C.byref(h)) == hprt.E_UNSUPPORTED and h.value is None
        assert err() == said and "nbDirections" in said and "object" not in said and "top level" not in said
    q = _params(hprt, "bspcluster", 4)
    q.chooser = 7
    assert fn(m._h, C.byref(q), C.byref(h)) == hprt.E_UNSUPPORTED and "unknown direction chooser" in err()
    with pytest.raises(ValueError):
        hprt.BspNodeInst(m, "bsppaper")
    # and a good build still follows a refused one
    assert hprt.BspNodeInst(m, "bspclusterwithkd", n_directions=4).info()["nodes"] >= 1


@pytest.mark.parametrize("fast", [False, True], ids=["plain", "fastkd"])
def test_the_two_level_depth_rule_is_the_handles(hprt, tmp_path, fast):
    """depth(top) + deepest object depth + 1 may be 64 and not 65 (CheckTwoLevelDepth's existing overload): hand-made staircases in
    place of the built trees of a BspNodeInst, as tests/test_bsppaperinst_host.py holds it for a BspPaperInst"""
    acc = "bsprandomfastkd" if fast else "bsprandom"
    pair = ns.deep_pair(fast)
    m, path = ns.bake(hprt, tmp_path, pair.text(), "deep")
    bi, ref = hprt.BspNodeInst(m, acc, n_directions=4), bsppaperinst_ref.BspPaperInstScene(path, fast)
    pair.install(bi, ref)
    inf = bi.info()
    assert inf["depth"] + inf["object_depth"] + 1 == deep_todo.CAPACITY == 64 and inf["kd_aware"] == int(fast)
    deeper = ns.deep_pair(fast, ns.bs.OBJECT_LEVELS + 1)
    m2, path2 = ns.bake(hprt, tmp_path, deeper.text(), "deeper")
    bi2, ref2 = hprt.BspNodeInst(m2, acc, n_directions=4), bsppaperinst_ref.BspPaperInstScene(path2, fast)
    before = bi2.object_copy(0)
    bi2.set_tree(-1, *deeper.trees()[-1], ref2.tree_bounds(-1))
    with pytest.raises(hprt.HprtError) as e:
        bi2.set_tree(0, *deeper.trees()[0], ref2.tree_bounds(0))
    assert e.value.code == hprt.E_UNSUPPORTED and "maxdepth" in str(e.value) and "(64 entries)" in str(e.value)
    assert bi2.object_copy(0)[0].tobytes() == before[0].tobytes()


def test_the_device_entry_without_a_device(hprt, own, simple, tmp_path):
    """hprt_bspnodeinst_build_device: the host entry's refusals first, with its codes and messages, then HPRT_E_NO_DEVICE and *out
    NULL where there is no HIP device (on a GPU machine: the host's bytes; tests/test_gpu_bspnodeinst.py holds more)"""
    import torch
    m, ref, _ = own
    host, dev = hprt.lib.hprt_bspnodeinst_build, hprt.lib.hprt_bspnodeinst_build_device
    flat, _ = ns.bake(hprt, tmp_path, ns.no_instances("bspcluster"), "flat")
    good, bad = _params(hprt, "bspclusterfastkd", 4), _params(hprt, "bspclusterfastkd", 2)
    st = hprt.BuildDeviceStats()
    h = C.c_void_p(0xdead)
    assert dev(None, C.byref(good), None, C.byref(st), C.byref(h)) == hprt.E_INVALID and h.value is None
    for model, q, code in ((flat, bad, hprt.E_UNSUPPORTED), (m, bad, hprt.E_UNSUPPORTED), (simple[0], None, hprt.E_INVALID)):
        h = C.c_void_p(0xdead)
        assert host(model._h, None if q is None else C.byref(q), C.byref(h)) == code
        said = hprt.lib.hprt_last_error().replace(b"hprt_bspnodeinst_build", b"hprt_bspnodeinst_build_device")
        h = C.c_void_p(0xdead)
        assert dev(model._h, None if q is None else C.byref(q), None, C.byref(st), C.byref(h)) == code and h.value is None
        assert hprt.lib.hprt_last_error() == said
    h = C.c_void_p(0xdead)
    rc = dev(m._h, C.byref(good), None, C.byref(st), C.byref(h))
    if torch.cuda.is_available():
        assert rc == 0 and h.value
        hprt.lib.hprt_bsppaperinst_destroy(h)
        nr.assert_same_trees(hprt.BspNodeInst(m, "bspclusterfastkd", n_directions=4, device=0, min_candidates=1), ref, "bspclusterfastkd", n_directions=4)
    else:
        assert rc == hprt.E_NO_DEVICE and h.value is None
        with pytest.raises(hprt.HprtError) as e:
            hprt.BspNodeInst(m, "bspclusterfastkd", n_directions=4, device=0, min_candidates=1)
        assert e.value.code == hprt.E_NO_DEVICE


def test_the_single_level_entries_and_the_front_ends_warning_are_unchanged(hprt, own):
    m, _, _ = own
    assert m.accelerator == "bspcluster"
    w = m.warnings()
    assert any('"bspcluster" is outside the hot-path scope; "bvh" used' in x for x in w), w
    assert not any("bspnodeinst" in x or "hprt_scene_attach_" in x for x in w), w
    for cls, acc in ((hprt.BspNode, "bspcluster"), (hprt.BspNodeKd, "bspclusterfastkd")):
        with pytest.raises(hprt.HprtError) as e:
            cls(m, acc)
        assert e.value.code == hprt.E_UNSUPPORTED
        assert str(e.value).endswith("node-based BSP trees over object instances are not supported (the scene keeps its BVH)"), str(e.value)
    with pytest.raises(hprt.HprtError) as e:
        hprt.bspnode_tree(m)                                          # stays single-level
    assert e.value.code == hprt.E_UNSUPPORTED
    hprt.Bvh(m)


# ---- the tie-free seeds (tests/bspnodeinst_fuzz.py) ----

_scenes = {}


def _scene(hprt, orc, d, seed):
    if seed not in _scenes:
        text = random_scene(seed, objects=2, twins=False)
        m, path = tf.bake(hprt, d, text, "s%d" % seed)
        oracle = orc.OracleScene(path)
        rays = tf.joined(tf.probe_rays(m, oracle, hprt.Bvh(m).info()["bounds"], seed))
        _scenes[seed] = (m, path, rays, oracle.intersect_inst(*rays)[:4])
    return _scenes[seed]


def test_the_seed_lists_are_complete():
    assert list(nf.CONFIGS) == ["bsprandominst", "bsprandomfastkdinst"] and (nf.K, nf.TREE_SEED) == (5, 7)
    for c in nf.CONFIGS.values():
        assert c.two_level and c.objects == 2 and c.attach == "attach_bsppaperinst" and len(set(c.film)) >= 3, c.name
    assert nf.CONFIGS["bsprandomfastkdinst"].kd_aware and not nf.CONFIGS["bsprandominst"].kd_aware


@pytest.mark.parametrize("name,seed", nf.FILM_PAIRS, ids=["%s-%d" % p for p in nf.FILM_PAIRS])
def test_tie_free_pair_loses_no_hit(hprt, orc, tmp_path_factory, name, seed):
    """on all 40,000 probe rays the restated two-level walk over the library's trees finds the oracle's t, primitive, instance and
    barycentrics"""
    c = nf.CONFIGS[name]
    if "dir" not in _scenes:
        _scenes["dir"] = tmp_path_factory.mktemp("bspnodeinst_fuzz")
    m, path, rays, (t0, p0, i0, b0) = _scene(hprt, orc, _scenes["dir"], seed)
    assert rays[0].shape[0] == 2 * tf.N_PROBE == 40000
    tree = c.make(hprt, m)
    assert tree.info()["kd_aware"] == int(c.kd_aware) and tree.info()["object_trees"] >= 1
    t1, p1, i1, b1 = c.closest(c.restate(path, tree), *rays)
    assert np.array_equal(p0, p1) and np.array_equal(i0, i1), (int((p0 != p1).sum()), int((i0 != i1).sum()))
    assert np.array_equal(_bits(t0), _bits(t1)) and np.array_equal(_bits(b0), _bits(b1))
    assert (p0 >= 0).sum() > 1000 and (i0 >= 0).sum() > 1000
