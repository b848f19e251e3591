"""Trees made by hand (the hprt_debug_<tree>_from_arrays hooks) and the staircase of tests/deep_todo.py, on the CPU: a built tree
survives arrays() -> from_arrays -> arrays() unchanged; a hand-made tree passes the checks a built tree passes (accepted at 64
levels, refused at 65, a child index out of range refused); and by the restatements' max_todo alone the staircase's rays hold the
todo entries they are aimed at — every level next to an LDS count, and the capacity.  The device walks are held to these
restatements in tests/test_gpu_deep_todo.py."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
import deep_todo as dt

DODECA = os.path.join(GOLDEN, "dodecahedron.hprt")


def _built(hprt, tree, source):
    """a built tree of either source, the primitives it is over and bounds to hand back with its arrays"""
    if source == "dodecahedron":
        m = hprt.Model.load(DODECA)
        n, bounds = m.counts()["primitives"], np.array(hprt.Bvh(m).info()["bounds"], np.float32)
        return {"kdtree": lambda: hprt.KdTree(m), "rbsp": lambda: hprt.Rbsp(m, n_directions=13), "rbspkd": lambda: hprt.RbspKd(m, n_directions=9),
                "bsppaper": lambda: hprt.BspPaper(m), "bsppaperkd": lambda: hprt.BspPaperKd(m)}[tree](), n, bounds
    p9 = np.random.default_rng(7).uniform(0, 1, (60, 9)).astype(np.float32)
    P = p9.reshape(-1, 3, 3)
    bounds = np.concatenate([P.reshape(-1, 3).min(0), P.reshape(-1, 3).max(0)])
    return {"kdtree": lambda: hprt.KdTree.from_bounds(P.min(1), P.max(1)), "rbsp": lambda: hprt.Rbsp.from_triangles(p9, n_directions=7),
            "rbspkd": lambda: hprt.RbspKd.from_triangles(p9, n_directions=13), "bsppaper": lambda: hprt.BspPaper.from_triangles(p9),
            "bsppaperkd": lambda: hprt.BspPaperKd.from_triangles(p9)}[tree](), 60, bounds


@pytest.mark.parametrize("source", ["dodecahedron", "soup"])
@pytest.mark.parametrize("tree", dt.TREES)
def test_a_built_tree_survives_the_round_trip(hprt, tree, source):
    t, n, bounds = _built(hprt, tree, source)
    nodes, idx = t.arrays()
    inf = t.info()
    extra = (inf["M"],) if "M" in inf else ()
    back = type(t).from_arrays(nodes, idx, n, bounds, *extra)
    n2, i2 = back.arrays()
    assert np.array_equal(nodes, n2) and np.array_equal(idx, i2) and nodes.shape[0] > 1
    assert all(back.info()[k] == inf[k] for k in ("nodes", "leaves", "prim_refs", "depth") + (("M",) if extra else ()))
    if extra:
        assert np.array_equal(back.directions().view(np.uint32), t.directions().view(np.uint32))


@pytest.mark.parametrize("tree", dt.TREES)
def test_the_staircase_is_accepted_at_64_levels_and_refused_at_65(hprt, tree):
    inf = dt.Staircase(64).handle(hprt, tree).info()
    assert inf["depth"] == 64 and inf["nodes"] == 255 and inf["leaves"] == 128
    with pytest.raises(hprt.HprtError) as e:
        dt.Staircase(65).handle(hprt, tree)
    assert e.value.code == hprt.E_UNSUPPORTED and "65" in str(e.value)


@pytest.mark.parametrize("tree", dt.TREES)
def test_a_child_index_out_of_range_is_refused(hprt, tree):
    st = dt.Staircase(9)
    nodes, idx = st.arrays(tree)
    cls = type(st.handle(hprt, tree))
    extra = {"rbsp": (dt.RBSP_M,), "rbspkd": (dt.RBSPKD_M,)}.get(tree, ())
    shift = {"kdtree": 2, "rbsp": 3, "rbspkd": 4, "bsppaper": 1, "bsppaperkd": 3}[tree]
    for above in (nodes.shape[0], 1, 0):         # past the array; the below child itself; the node itself
        bad = nodes.copy()
        bad[0, 1] = (bad[0, 1] & ((1 << shift) - 1)) | (above << shift)
        with pytest.raises(hprt.HprtError) as e:
            cls.from_arrays(bad, idx, st.n_prims, st.bounds, *extra)
        assert e.value.code == hprt.E_INVALID, above
    bad = nodes.copy()
    bad[2, 0] = st.n_prims                        # a one-primitive leaf naming a primitive past the last
    with pytest.raises(hprt.HprtError) as e:
        cls.from_arrays(bad, idx, st.n_prims, st.bounds, *extra)
    assert e.value.code == hprt.E_INVALID
    with pytest.raises(hprt.HprtError) as e:      # the last leaf's range runs past primitiveIndices
        cls.from_arrays(nodes, idx[:1], st.n_prims, st.bounds, *extra)
    assert e.value.code == hprt.E_INVALID


@pytest.fixture(scope="module", params=[64, 9, 8])
def baked(request, hprt, tmp_path_factory):
    st = dt.Staircase(request.param)
    return st, st.bake(hprt, tmp_path_factory.mktemp("staircase"))


def test_the_staircase_has_no_ties(baked):
    dt.check_no_ties(baked[0])


@pytest.mark.parametrize("any_hit", [False, True], ids=["closest", "any"])
@pytest.mark.parametrize("tree", dt.TREES)
def test_the_ray_families_hold_the_entries_they_are_aimed_at(baked, tree, any_hit):
    """On the restatement alone: every level of deep_todo.LEVELS (those the staircase has) is the deepest of at least 1/32 of the
    rays, at 64 levels some ray holds all 64 entries, at 9 levels the ninth entry is reached and at 8 it is not, and the control
    family never holds more than one."""
    st, path = baked
    ref = st.reference(tree, path)
    assert np.array_equal(ref.triangles().reshape(-1, 3, 3), st.tris)      # the baked file holds the generator's triangles, in its order
    mt = dt.check_ray_family(st, ref, any_hit=any_hit)
    assert (mt > 8).any() == (st.L > 8)
    if tree == "rbspkd" and st.L == 64:      # the dot-product step crosses the seam too: a push at an oblique sibling node lands past entry 8
        o, d, tm, _ = st.deep_rays(4096)
        (ref.occluded if any_hit else ref.intersect)(o, d, tm)
        assert (ref.max_todo_dot() > 8).any()


# ---- the sixth form: the binary BVH chain (k_trace) and its four-wide collapse (k_walk4) ----
def _creation_hits(hprt, stairs, path, o, d, tm):
    """the kd restatement's closest hits on the staircase's triangles as creation-order triangle numbers, and its occlusion"""
    ref = stairs.reference("kdtree", path)
    t, p, b, _ = ref.intersect(o, d, tm)
    order = hprt.Bvh(hprt.Model.load(path)).arrays()[1].astype(np.int64)      # the restatement numbers hits in the scene's BVH order
    return t, np.where(p >= 0, order[np.maximum(p, 0)], -1), b, ref.occluded(o, d, tm)[0]


def test_the_bvh_chain_holds_the_entries_its_rays_are_aimed_at(hprt, tmp_path):
    """The §2 conditions for the binary chain, from the replay of BVHAccel::Intersect alone: each of 1, 7, 8, 9, 10, 12, 13, 16, 17,
    20, 21, 33 and 63 is the deepest of at least 1/32 of the rays and some ray holds 63 entries: the binary limit is 63 interior
    levels (deep_todo.BvhChain), so 63 stands for the issue's 63 and 64.  The replay's hits are the kd restatement's on the same
    triangles: the construction has no ties, and the replay's exact triangle test decides as the float test does."""
    chain = dt.BvhChain()
    dt.check_no_ties(chain.stairs)
    level = dt.check_bvh_family(chain)
    assert chain.N == 63 and set(chain.levels()) >= {1, 7, 8, 9, 10, 12, 13, 16, 17, 20, 21, 33, 63}
    o, d, tm, _ = chain.deep_rays(4096)
    _, want, _, occ = _creation_hits(hprt, chain.stairs, chain.stairs.bake(hprt, tmp_path), o, d, tm)
    assert np.array_equal(chain.replay(o, d, tm)[1], want) and 0.05 < (want >= 0).mean() < 0.95
    assert np.array_equal(chain.replay(o, d, tm, any_hit=True)[1], occ)


def test_the_wide_chain_reaches_stack_need(hprt):
    """k_walk4 over the collapse of a 60-level chain: hprt_debug_wide_build reports stack_need = 60, which is > 20 and the walk's
    capacity; by the replay of the wide walk, 12, 13, 20 and 21 entries (its LDS counts and one past) are each the deepest of at
    least 1/32 of the rays, and some ray holds exactly stack_need."""
    chain = dt.BvhChain(dt.WIDE_CHAIN)
    wide, need = chain.wide(hprt)
    assert 20 < need <= 60 and need == dt.WIDE_CHAIN
    o, d, tm, level = chain.deep_rays(1024)
    deep = dt.wide_depths(chain, wide, o, d, tm)
    for m in (12, 13, 20, 21):
        assert (deep == m).mean() >= 1 / 32, (m, (deep == m).mean())
    assert deep.max() == need and (deep <= level).all()
