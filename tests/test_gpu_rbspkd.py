"""The rbspkd walk on the GPU (Accelerator "rbspkd"): closest and any hit held bit for bit to the test-side restatement of
RBSPKd::Intersect / IntersectP (tests/rbspkd_reference.cpp over tests/tree_reference.h) — t, primitive, barycentrics, all four
counters and the kd share — on camera, random, degenerate, infinite and on-a-split-plane rays, including rays built so that the
kd form of an axis node and RBSP's dot-product form disagree; renders against the reference's images; per-pixel kd statistics;
tile sharding; switching between the kd, RBSP and rbspkd walks; attach refusals; kernel resources.  The checks shared with the
other tree walks are tests/tree_walk_checks.py's."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, KILLEROO
from tree_ref import rbspkd as rbspkd_ref
import tree_walk_checks as twc
from tree_walk_checks import _bits

pytestmark = pytest.mark.gpu
DODECA = os.path.join(GOLDEN, "dodecahedron.hprt")
CASES = [(DODECA, 3), (DODECA, 7), (DODECA, 9), (DODECA, 13), (KILLEROO, 3), (KILLEROO, 7)]


@pytest.fixture(scope="module", params=CASES, ids=["dodecahedron-3", "dodecahedron-7", "dodecahedron-9", "dodecahedron-13", "killeroo-simple-3",
                                                   "killeroo-simple-7"])
def rk(request, hprt, orc):
    path, M = request.param
    m = hprt.Model.load(path)
    bvh = hprt.Bvh(m)
    sc = hprt.Scene(m, bvh, device=0)
    tree = hprt.RbspKd(m, n_directions=M)
    sc.attach_rbspkd(tree)
    if path == DODECA:
        ref = rbspkd_ref.RbspKdScene(path, M)                 # the restated build: the library's tree must be the same
        nodes, idx = tree.arrays()
        rn, ri = ref.tree()
        assert np.array_equal(nodes, rn) and np.array_equal(idx, ri)
    else:
        ref = rbspkd_ref.RbspKdScene(path, M, build=False)   # killeroo-simple's restated build is slow: walk the library's tree
        ref.set_tree(*tree.arrays())
    b = np.array(bvh.info()["bounds"], np.float32)
    return path, M, m, sc, tree, ref, orc.OracleScene(path), (b[:3], b[3:])


def _splits(tree):
    """(direction, split position) of every interior node of the tree"""
    nodes, _ = tree.arrays()
    M = tree.info()["M"]
    mask = (1 << M.bit_length()) - 1
    ax = nodes[:, 1] & mask
    inner = ax != M
    return ax[inner].astype(np.int64), nodes[inner, 0].view(np.float32)


def _rays(tree, ref, oracle, bounds, n, seed):
    rng = np.random.default_rng(seed)
    blo, bhi = bounds
    ext = bhi - blo
    # origins exactly on split planes, oblique ones included (float Dot(dir, o) == split)
    ax, pos = _splits(tree)
    return [twc.camera_rays(rng, oracle, n), twc.random_rays(rng, blo, ext, n), twc.degenerate_rays(rng, blo, ext, n),
            twc.plane_tie_rays(rng, blo, ext, n, tree.directions()[ax], pos), _separating_rays(tree, bounds, n, rng)]


def _separating_rays(tree, bounds, n, rng):
    """Rays on which the kd form of an axis node and the dot-product form disagree: origins exactly on the tree's own axis
    splits with d[axis] = +-0 (kd: belowFirst; dot: 1 / (+0) = +inf, not below first) or +-inf, and origins with a +-inf or -0
    component off the axis (the dot product turns 0 * inf into NaN)."""
    blo, bhi = bounds
    ext = bhi - blo
    ax, pos = _splits(tree)
    kd = ax < 3
    if not kd.any():
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros(0, np.float32)
    ax, pos = ax[kd], pos[kd]
    pick = rng.integers(0, ax.shape[0], n)
    a, p = ax[pick], pos[pick]
    rows = np.arange(n)
    o = (blo + rng.uniform(0, 1, (n, 3)) * ext).astype(np.float32)
    o[rows, a] = p
    d = rng.normal(size=(n, 3)).astype(np.float32)
    q = n // 6
    d[rows[:q], a[:q]] = 0.0
    d[rows[q:2 * q], a[q:2 * q]] = -0.0
    d[rows[2 * q:3 * q], a[2 * q:3 * q]] = np.inf
    d[rows[3 * q:4 * q], a[3 * q:4 * q]] = -np.inf
    other = (a + 1) % 3
    o[rows[4 * q:5 * q], other[4 * q:5 * q]] = np.where(rng.uniform(size=q) < 0.5, np.float32(np.inf), np.float32(-np.inf))
    o[rows[5 * q:], other[5 * q:]] = -0.0
    d[rows[5 * q:], a[5 * q:]] = np.where(rng.uniform(size=n - 5 * q) < 0.5, np.float32(0.0), np.float32(-0.0))
    return o, d, np.full(n, np.inf, np.float32)


def test_closest_hit_equals_the_reference_walk(rk):
    _, _, _, sc, tree, ref, oracle, bounds = rk
    # (a tree without axis nodes has no separating rays)
    twc.check_closest(sc, ref, [r for r in _rays(tree, ref, oracle, bounds, 20000, 1) if r[2].shape[0]])


def test_any_hit_equals_the_reference_walk(rk):
    _, _, _, sc, tree, ref, oracle, bounds = rk
    twc.check_any(sc, ref, [r for r in _rays(tree, ref, oracle, bounds, 20000, 2) if r[2].shape[0]])


def test_separating_rays_tell_the_kd_form_from_the_dot_form(rk):
    """On the separating rays the device follows the kd form; RBSP's dot-product step (the restatement with dot_only, the
    step k_rbspwalk takes) walks some of them differently, so a walk with that step would fail here."""
    _, _, _, sc, tree, ref, _, bounds = rk
    if tree.info()["kd_interior"] == 0:
        pytest.skip("no axis nodes")
    o, d, tm = _separating_rays(tree, bounds, 20000, np.random.default_rng(5))
    t0, p0, b0, c0 = ref.intersect(o, d, tm)
    occ0, q0 = ref.occluded(o, d, tm)
    t1, p1, b1, c1 = sc.intersect(o, d, tm, count=True)
    assert np.array_equal(p0, p1) and np.array_equal(_bits(t0), _bits(t1)) and np.array_equal(_bits(b0), _bits(b1))
    assert c1.tolist() == c0[:, :4].sum(0).tolist()
    occ1, q1 = sc.occluded(o, d, tm, count=True)
    assert np.array_equal(occ0, occ1) and q1.tolist() == q0[:, :4].sum(0).tolist()
    ref.dot_only(True)
    try:
        t2, p2, b2, c2 = ref.intersect(o, d, tm)
        occ2, q2 = ref.occluded(o, d, tm)
    finally:
        ref.dot_only(False)
    differs = (c2 != c0).any(1) | (q2 != q0).any(1) | (p2 != p0) | (_bits(t2) != _bits(t0)) | (occ2 != occ0)
    assert differs.sum() > 0, "no separating ray separates the two forms"


def test_device_entry_points_agree_with_the_host_ones(rk):
    _, _, _, sc, tree, ref, oracle, bounds = rk
    twc.check_device_entry_points(sc, *_rays(tree, ref, oracle, bounds, 4096, 3)[1])


def test_rbspkd_renders_match_the_reference_images(hprt, rk):
    path, _, m, sc, _, _, _, _ = rk
    twc.check_reference_image(hprt, sc, m, path)


def test_counting_render_pixel_kd_stats(hprt, rk, tmp_path):
    _, M, m, sc, _, _, _, _ = rk
    st, px, check_plain_film = twc.check_counting_render(sc, m)
    kdc = sc.kd_counters()
    kd2 = sc.pixel_kd_stats()
    assert int(kd2[0].sum()) == kdc[0] and int(kd2[1].sum()) == kdc[1]
    assert (kd2[0] <= px[:, :, 5]).all() and (kd2[1] <= px[:, :, 6]).all()
    assert kdc[0] > 0 and kdc[1] > 0
    if M == 3:
        assert kdc == (st["nodes_entered"], st["nodes_entered_p"])
    hprt.write_pixel_stats_rbspkd(str(tmp_path / "rk"), px, kd2)
    load = lambda n: np.loadtxt(tmp_path / ("rk-%s.txt" % n), dtype=np.uint64).reshape(px.shape[:2])
    assert np.array_equal(load("kdTreeNodeTraversals"), kd2[0]) and np.array_equal(load("kdTreeNodeTraversalsP"), kd2[1])
    assert np.array_equal(load("bspTreeNodeTraversals"), px[:, :, 5] - kd2[0])
    assert np.array_equal(load("bspTreeNodeTraversalsP"), px[:, :, 6] - kd2[1])
    check_plain_film()


def test_tile_sharded_rbspkd_render_merges_bit_identically(hprt, rk):
    _, _, m, sc, _, _, _, _ = rk
    twc.check_tile_sharding(hprt, sc, m)


def test_attaching_any_tree_replaces_the_others(hprt):
    """kd -> rbsp -> rbspkd -> kd on one scene: each render is the one a scene with only that tree gives, with its counters."""
    m = hprt.Model.load(DODECA)
    opt = m.options.copy(); opt.spp = 2
    trees = {"kd": ("attach_kdtree", hprt.KdTree(m)), "rbsp": ("attach_rbsp", hprt.Rbsp(m, n_directions=7)),
             "rbspkd": ("attach_rbspkd", hprt.RbspKd(m, n_directions=7))}
    alone = {}
    for name, (attach, tree) in trees.items():
        s = hprt.Scene(m, hprt.Bvh(m), device=0)
        getattr(s, attach)(tree)
        alone[name] = s.render(opt, count_work=True) + (s.kd_counters(),)
    assert alone["rbsp"][1]["nodes_entered"] != alone["rbspkd"][1]["nodes_entered"]
    assert alone["rbsp"][2] == (0, 0) and alone["rbspkd"][2][0] > 0
    sc = hprt.Scene(m, hprt.Bvh(m), device=0)
    for name in ("kd", "rbsp", "rbspkd", "kd"):
        attach, tree = trees[name]
        getattr(sc, attach)(tree)
        film, st = sc.render(opt, count_work=True)
        assert np.array_equal(film.view(np.uint32), alone[name][0].view(np.uint32)), name
        assert st["nodes_entered"] == alone[name][1]["nodes_entered"] and st["nodes_fetched"] == alone[name][1]["nodes_fetched"], name
        assert sc.kd_counters() == alone[name][2], name


def test_attach_refusals(hprt):
    m = hprt.Model.load(DODECA)
    sc = hprt.Scene(m, hprt.Bvh(m), device=0)
    rng = np.random.default_rng(0)
    with pytest.raises(hprt.HprtError) as e:
        sc.attach_rbspkd(hprt.RbspKd.from_triangles(rng.uniform(0, 1, (7, 9))))     # not this scene's primitive count
    assert e.value.code == hprt.E_INVALID
    mi = hprt.Model.load(os.path.join(GOLDEN, "simple_instanced.hprt"))
    si = hprt.Scene(mi, hprt.Bvh(mi), device=0)
    with pytest.raises(hprt.HprtError) as e:
        si.attach_rbspkd(hprt.RbspKd.from_triangles(rng.uniform(0, 1, (1, 9))))
    assert e.value.code == hprt.E_UNSUPPORTED
    opt = m.options.copy(); opt.spp = 1
    sc.render(opt)                                       # no rbspkd tree and no pixel statistics: nothing to read
    with pytest.raises(hprt.HprtError) as e:
        sc.pixel_kd_stats()
    assert e.value.code == hprt.E_INVALID


def test_rbspkd_walk_resources(hprt, tmp_path):
    """k_rbspkdwalk's targets are k_rbspwalk's: triangle-only kernels <= 80 registers (six workgroups per CU) with nothing in
    scratch, quadric kernels <= 128 (four); LDS: eight todo entries per lane of a 256-thread workgroup plus the direction table."""
    twc.check_walk_resources(tmp_path, "k_rbspkdwalk", 8 * 256 * 8 + 4 * 3 * 13)
