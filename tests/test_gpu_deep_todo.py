"""The tree walks' todo lists past their LDS entries, up to capacity: k_kdwalk, k_rbspwalk, k_rbspkdwalk, k_bsppaperwalk and
k_bsppaperkdwalk keep 8 entries per lane in LDS and the rest, up to 64, in the scene's deep-stack area in HBM ([entry][grid thread]).
The staircase of tests/deep_todo.py gives every ray a known number of entries (tests/test_deep_todo_host.py asserts that on the
restatements alone); here each device walk over the hand-made tree is held bit for bit to its restatement walking the same arrays —
primitive, t, barycentrics, all counters and the kd share — at 64 levels (rays at every level next to an LDS count and at the
capacity, mixed within every wave), at 9 and 8 levels (the smallest trees where the seam is and is not crossed: a failure says
which side broke), with 917,504 rays (twice the deep-stack stride, so that the slots of a full persistent grid are live together),
with a sphere in the last leaf (the QUAD instantiations) and through a render (the queue-driven launches).

The BVH walks share the spill area: k_trace (16 / 10 / 7 LDS entries of 64) over a binary chain of 63 interior levels given through
SceneDesc, and k_walk4 (12 / 20 of 60) over the collapse of a 60-level chain, whose stack_need is exactly 60."""
import ctypes as C

import numpy as np
import pytest

import deep_todo as dt
import tree_walk_checks as twc

pytestmark = pytest.mark.gpu
ATTACH = {"kdtree": "attach_kdtree", "rbsp": "attach_rbsp", "rbspkd": "attach_rbspkd", "bsppaper": "attach_bsppaper", "bsppaperkd": "attach_bsppaperkd"}
DEEP_THREADS = 458752      # HPRT_DEEP_THREADS: the stride of the deep-stack area, the threads of the largest persistent grid
_BAKED, _WALKS = {}, {}


def _baked(hprt, tmp_path_factory, L, sphere=False):
    """(staircase, path of its baked scene, model), once per module"""
    if (L, sphere) not in _BAKED:
        st = dt.Staircase(L, sphere=sphere)
        path = st.bake(hprt, tmp_path_factory.mktemp("staircase"))
        _BAKED[L, sphere] = (st, path, hprt.Model.load(path))
    return _BAKED[L, sphere]


def _walk(hprt, tmp_path_factory, tree, L, sphere=False):
    """(staircase, scene with the hand-made tree attached, restatement over the same arrays), once per module"""
    if (tree, L, sphere) not in _WALKS:
        st, path, m = _baked(hprt, tmp_path_factory, L, sphere)
        sc = hprt.Scene(m, hprt.Bvh(m), device=0)
        getattr(sc, ATTACH[tree])(st.handle(hprt, tree))
        _WALKS[tree, L, sphere] = (st, sc, st.reference(tree, path))
    return _WALKS[tree, L, sphere]


def _plain_closest(sc, ref, o, d, tm):
    """the kernels without counters (another instantiation) return the same hits"""
    t0, p0, b0, _ = ref.intersect(o, d, tm)
    t1, p1, b1 = sc.intersect(o, d, tm)
    assert np.array_equal(p0, p1), int((p0 != p1).sum())
    assert np.array_equal(twc._bits(t0), twc._bits(t1)) and np.array_equal(twc._bits(b0), twc._bits(b1))


@pytest.mark.parametrize("L", [64, 9, 8])
@pytest.mark.parametrize("tree", dt.TREES)
def test_closest_hit_across_the_seam(hprt, tmp_path_factory, tree, L):
    st, sc, ref = _walk(hprt, tmp_path_factory, tree, L)
    o, d, tm, level = st.deep_rays(16384)
    twc.check_closest(sc, ref, [(o, d, tm), st.control_rays(4096)])
    assert ref.max_todo().max() == 1      # the control family, walked last
    _plain_closest(sc, ref, o, d, tm)
    assert np.array_equal(ref.max_todo(), level) and level.max() == L


@pytest.mark.parametrize("L", [64, 9, 8])
@pytest.mark.parametrize("tree", dt.TREES)
def test_any_hit_across_the_seam(hprt, tmp_path_factory, tree, L):
    st, sc, ref = _walk(hprt, tmp_path_factory, tree, L)
    o, d, tm, level = st.deep_rays(16384, seed=3)
    twc.check_any(sc, ref, [st.control_rays(4096, seed=4), (o, d, tm)])
    assert np.array_equal(ref.max_todo(), level) and level.max() == L
    occ0, _ = ref.occluded(o, d, tm)
    assert np.array_equal(occ0, sc.occluded(o, d, tm)) and 0 < occ0.mean() < 1


@pytest.mark.parametrize("tree", dt.TREES)
def test_a_full_grid_of_deep_lanes(hprt, tmp_path_factory, tree):
    """2 x HPRT_DEEP_THREADS rays in one launch: 16,384 rays of the deep family tiled 56 times (the restatement walks them once), so
    that every workgroup of the largest persistent grid has lanes in its deep-stack slots while its neighbours do.  Hits, and the
    counters summed, are 56 times the restatement's."""
    st, sc, ref = _walk(hprt, tmp_path_factory, tree, 64)
    o, d, tm, level = st.deep_rays(16384, seed=5)
    reps = 2 * DEEP_THREADS // 16384
    assert reps * 16384 == 2 * DEEP_THREADS and (level > 8).mean() == 53 / 64      # of every 64 rays, 4 + 4 + 3 aim at levels 1, 7 and 8
    t0, p0, b0, c0 = ref.intersect(o, d, tm)
    t1, p1, b1, c1 = sc.intersect(np.tile(o, (reps, 1)), np.tile(d, (reps, 1)), np.tile(tm, reps), count=True)
    assert np.array_equal(p1, np.tile(p0, reps)), int((p1 != np.tile(p0, reps)).sum())
    assert np.array_equal(twc._bits(t1), np.tile(twc._bits(t0), reps)) and np.array_equal(twc._bits(b1), np.tile(twc._bits(b0), (reps, 1)))
    assert c1.tolist() == (reps * c0[:, :4].sum(0)).tolist(), (c1, reps * c0.sum(0))
    if c0.shape[1] == 5:
        assert sc.kd_counters() == (reps * int(c0[:, 4].sum()), 0)


@pytest.mark.parametrize("tree", dt.TREES)
def test_quadric_variants_across_the_seam(hprt, tmp_path_factory, tree):
    """a sphere in the last leaf: the QUAD kernels (another register allocation) hold 64 entries too"""
    st, sc, ref = _walk(hprt, tmp_path_factory, tree, 64, sphere=True)
    o, d, tm, level = st.deep_rays(16384, seed=6)
    twc.check_closest(sc, ref, [(o, d, tm)])
    assert np.array_equal(ref.max_todo(), level)
    twc.check_any(sc, ref, [(o, d, tm)])
    _, _, _, c = sc.intersect(o, d, tm, count=True)
    assert c[3] > 0      # sphere tests: the QUAD kernels walked


@pytest.mark.parametrize("tree", dt.TREES)
def test_another_primitive_count_is_refused_at_attach(hprt, tmp_path_factory, tree):
    """(A GPU test although it is a refusal: hprt_scene_attach_* takes a device scene, and hprt_scene_create needs a device.)
    A hand-made tree is checked at attach like any other: the 9-level staircase's tree does not fit the 8-level scene, which
    keeps the tree it has"""
    st, sc, ref = _walk(hprt, tmp_path_factory, tree, 8)
    with pytest.raises(hprt.HprtError) as e:
        getattr(sc, ATTACH[tree])(dt.Staircase(9).handle(hprt, tree))
    assert e.value.code == hprt.E_INVALID
    o, d, tm, _ = st.deep_rays(1024, seed=7)
    _plain_closest(sc, ref, o, d, tm)


@pytest.mark.parametrize("tree", ["kdtree", "bsppaperkd"])
def test_renders_across_the_seam(hprt, orc, tmp_path_factory, tree):
    """The queue-driven launches of a render (queue and count on the device): the camera looks down -x, so by the restatement every
    camera ray of the crop holds more than 8 entries.  The film of a counting and of a plain render is the BVH scene's bit for bit
    (the hits do not depend on the accelerator: deep_todo.check_no_ties), and the per-pixel statistics sum to the render's counters."""
    st, path, m = _baked(hprt, tmp_path_factory, 64)
    _, sc, ref = _walk(hprt, tmp_path_factory, tree, 64)
    dt.check_no_ties(st)
    px, py = np.meshgrid(np.arange(280, 328), np.arange(315, 355))
    o, d = orc.OracleScene(path).camera_rays(px.ravel().astype(np.int32), py.ravel().astype(np.int32), np.zeros(px.size, np.int64))
    _, p, _, _ = ref.intersect(o, d, np.full(px.size, np.inf, np.float32))
    assert ref.max_todo().min() > 8 and ref.max_todo().max() == 64 and 0.2 < (p >= 0).mean() < 0.9
    bvh = hprt.Scene(m, hprt.Bvh(m), device=0)
    st_, px_stats, check_plain_film = twc.check_counting_render(sc, m)
    opt = m.options.copy()
    opt.spp = 2
    for i, c in enumerate((0.4, 0.4 + 48 / 700.0, 0.45, 0.45 + 40 / 700.0)):      # check_counting_render's crop
        opt.crop[i] = c
    counted, _ = sc.render(opt, count_work=True)
    want_counted, _ = bvh.render(opt, count_work=True)
    assert np.array_equal(counted.view(np.uint32), want_counted.view(np.uint32))
    plain, _ = sc.render(opt)
    want_plain, _ = bvh.render(opt)
    assert np.array_equal(plain.view(np.uint32), want_plain.view(np.uint32)) and plain.max() > 0
    check_plain_film()


@pytest.mark.parametrize("N", [dt.BVH_CHAIN, dt.WIDE_CHAIN])
def test_the_bvh_walks_across_the_seam(hprt, tmp_path_factory, N):
    """The binary chain through SceneDesc.  k_trace (hprt_debug_wide_walk(0)), closest and any hit with counters: hits bit for bit the kd
    restatement's on the same triangles (accelerator-independent: deep_todo.check_no_ties), the four counters those of a plain
    Python replay of BVHAccel::Intersect / IntersectP over the chain.  k_walk4 (plain calls) over the collapse: the same hits, and
    the two walks agree.  At N = 63 k_trace holds up to 63 entries; at N = 60 k_walk4 holds exactly its stack_need = 60."""
    chain = dt.BvhChain(N)
    sc = chain.scene(hprt, device=0)
    _, need = chain.wide(hprt)
    assert need == N
    o, d, tm, level = chain.deep_rays(4096)
    path = chain.stairs.bake(hprt, tmp_path_factory.mktemp("chain"))
    ref = chain.stairs.reference("kdtree", path)
    t0, p0, b0, _ = ref.intersect(o, d, tm)
    order = hprt.Bvh(hprt.Model.load(path)).arrays()[1].astype(np.int64)      # the restatement numbers hits in that scene's BVH order
    want = np.where(p0 >= 0, order[np.maximum(p0, 0)], -1)                   # the chain's ordered numbers are creation numbers
    occ0, _ = ref.occluded(o, d, tm)
    c_closest, hit, deepest = chain.replay(o, d, tm)
    c_any, occ_r, _ = chain.replay(o, d, tm, any_hit=True)
    assert np.array_equal(hit, want) and np.array_equal(occ_r, occ0) and np.array_equal(deepest, level) and level.max() == N
    walk = hprt.lib.hprt_debug_scene_walk; walk.argtypes = [C.c_void_p]; walk.restype = C.c_int
    hprt.lib.hprt_debug_wide_walk.argtypes = [C.c_int]
    try:
        hprt.lib.hprt_debug_wide_walk(0)
        assert walk(sc._h) == 0
        t1, p1, b1, c1 = sc.intersect(o, d, tm, count=True)
        print("k_trace closest", c1.tolist(), c_closest.tolist())
        assert np.array_equal(p1, want), int((p1 != want).sum())
        assert np.array_equal(twc._bits(t1), twc._bits(t0)) and np.array_equal(twc._bits(b1), twc._bits(b0))
        assert c1.tolist() == c_closest.tolist(), (c1, c_closest)
        occ1, c2 = sc.occluded(o, d, tm, count=True)
        print("k_trace any", c2.tolist(), c_any.tolist())
        assert np.array_equal(occ1, occ0) and c2.tolist() == c_any.tolist(), (c2, c_any)
        t2, p2, b2 = sc.intersect(o, d, tm)                                   # k_trace without counters
        assert np.array_equal(p2, want) and np.array_equal(twc._bits(t2), twc._bits(t0)) and np.array_equal(twc._bits(b2), twc._bits(b0))
        assert np.array_equal(sc.occluded(o, d, tm), occ0)
        hprt.lib.hprt_debug_wide_walk(1)
        if N <= 60:                                                           # (a chain that needs more than 60 entries keeps the binary walk)
            assert walk(sc._h) == 1
        t3, p3, b3 = sc.intersect(o, d, tm)
        assert np.array_equal(p3, want), int((p3 != want).sum())
        assert np.array_equal(twc._bits(t3), twc._bits(t0)) and np.array_equal(twc._bits(b3), twc._bits(b0))
        assert np.array_equal(sc.occluded(o, d, tm), occ0)
    finally:
        hprt.lib.hprt_debug_wide_walk(-1)
    assert 0.05 < (want >= 0).mean() < 0.95 and 0.05 < occ0.mean() < 0.95
