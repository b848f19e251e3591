"""The kd-aware general BSP walk on the GPU (Accelerator "bsppaperkd"): closest and any hit held bit for bit to the test-side
restatement of BSPKd::Intersect / IntersectP (tests/bsppaperkd_reference.cpp) — t, primitive, barycentrics, all four counters and
the kd share, on every ray — on camera, random, degenerate and on-a-split-plane rays (kd splits and plane splits of the tree
itself), and on rays built so that the kd form of a kd node and the dot-product form disagree; renders against the reference's
images; per-pixel kd / bsp statistics; tile sharding; switching among the BVH and all five trees; attach refusals; the C++ host
example; kernel resources.  Scenes: the dodecahedron and a prefix of killeroo-simple's triangles with three spheres (the
restated build must equal the library's), and killeroo-simple (about two minutes to build on 16 threads; the restatement walks
the library's tree).  The checks shared with the other tree walks are tests/tree_walk_checks.py's."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import bsppaperkd_ref as kdref
import tree_walk_checks as twc
from tree_walk_checks import _bits

pytestmark = pytest.mark.gpu
DODECA = os.path.join(GOLDEN, "dodecahedron.hprt")
KILLEROO = os.path.join(GOLDEN, "killeroo_simple.hprt")
_SCENES = {}


def _scene(name, hprt, orc, tmp_path_factory):
    """(path, model, scene with the attached bsppaperkd tree, tree, restatement, oracle or None, BVH bounds), built once per module"""
    if name in _SCENES:
        return _SCENES[name]
    if name == "killeroo-prefix-spheres":
        from test_gpu_bsppaper import _prefix_scene
        path = _prefix_scene(tmp_path_factory, hprt)
    else:
        path = {"dodecahedron": DODECA, "killeroo-simple": KILLEROO}[name]
    m = hprt.Model.load(path)
    bvh = hprt.Bvh(m)
    sc = hprt.Scene(m, bvh, device=0)
    tree = hprt.BspPaperKd(m)
    sc.attach_bsppaperkd(tree)
    nodes, idx = tree.arrays()
    if name != "killeroo-simple":
        ref = kdref.BspKdScene(path)                      # the restated build: the library's tree must be the same
        kdref.assert_same_tree((nodes, idx), ref.tree())
    else:
        ref = kdref.BspKdScene(path, build=False)         # killeroo-simple's restated build is slow: walk the library's tree
        ref.set_tree(nodes, idx)
    b = np.array(bvh.info()["bounds"], np.float32)
    _SCENES[name] = (path, m, sc, tree, ref, orc.OracleScene(path) if name != "killeroo-prefix-spheres" else None, (b[:3], b[3:]))
    return _SCENES[name]


@pytest.fixture(scope="module", params=["dodecahedron", "killeroo-simple", "killeroo-prefix-spheres"])
def walked(request, hprt, orc, tmp_path_factory):
    """the scenes the walks are held to the restatement on"""
    return _scene(request.param, hprt, orc, tmp_path_factory)


@pytest.fixture(scope="module", params=["dodecahedron", "killeroo-simple"])
def bk(request, hprt, orc, tmp_path_factory):
    """the scenes with the reference's camera and image"""
    return _scene(request.param, hprt, orc, tmp_path_factory)


@pytest.fixture(scope="module")
def quad(hprt, orc, tmp_path_factory):
    return _scene("killeroo-prefix-spheres", hprt, orc, tmp_path_factory)


def _split_planes(tree):
    """(axes [P, 3], positions [P]) of the tree's interior nodes: the unit axis of a kd node, the stored axis of a plane node; and
    the kd nodes' (axis number, position)"""
    nodes, _ = tree.arrays()
    kind = nodes[:, 1] & kdref.KIND_MASK
    kd, plane = kind < kdref.LEAF, kind == kdref.PLANE
    axes = np.concatenate([np.eye(3, dtype=np.float32)[kind[kd]], nodes[plane, 2:].view(np.float32)])
    pos = np.concatenate([nodes[kd, 0].view(np.float32), nodes[plane, 0].view(np.float32)])
    return axes, pos, kind[kd].astype(np.int64), nodes[kd, 0].view(np.float32)


def _separating_rays(tree, bounds, n, rng):
    """Rays on which the kd form of a kd node and the dot-product form disagree: origins exactly on the tree's own kd splits with
    d[axis] = +-0 (kd: belowFirst; dot: 1 / (+0) = +inf, not below first) or +-inf, and origins with a +-inf or -0 component off
    the axis (the dot product turns 0 * inf into NaN)."""
    blo, bhi = bounds
    ext = bhi - blo
    _, _, ax, pos = _split_planes(tree)
    assert ax.shape[0] > 0
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


def _rays(tree, oracle, bounds, n, seed):
    rng = np.random.default_rng(seed)
    blo, bhi = bounds
    ext = bhi - blo
    out = [twc.camera_rays(rng, oracle, n)] if oracle is not None else []
    out += [twc.random_rays(rng, blo, ext, n), twc.degenerate_rays(rng, blo, ext, n)]
    # origins whose float Dot(axis, o) equals a node's split exactly (the belowFirst tie), on kd splits and plane splits alike
    axes, pos, _, _ = _split_planes(tree)
    out.append(twc.plane_tie_rays(rng, blo, ext, n, axes, pos))
    out.append(_separating_rays(tree, bounds, n, rng))
    return out


def test_walked_trees_hold_both_node_kinds(walked):
    """every walked tree has kd nodes and plane nodes, so both interior forms are exercised"""
    _, _, _, tree, _, _, _ = walked
    inf = tree.info()
    assert inf["kd_interior"] > 0 and inf["plane_interior"] > 0, inf
    _, kd, plane, leaves = kdref.kinds(tree.arrays()[0])
    assert (kd, plane, leaves) == (inf["kd_interior"], inf["plane_interior"], inf["leaves"])


def test_closest_hit_equals_the_reference_walk(walked):
    _, _, sc, tree, ref, oracle, bounds = walked
    twc.check_closest(sc, ref, _rays(tree, oracle, bounds, 20000, 1))


def test_any_hit_equals_the_reference_walk(walked):
    _, _, sc, tree, ref, oracle, bounds = walked
    twc.check_any(sc, ref, _rays(tree, oracle, bounds, 20000, 2))


def test_separating_rays_tell_the_kd_form_from_the_dot_form(walked):
    """On the separating rays the device follows the kd form; the dot-product step at every node (the restatement with dot_only,
    the step k_bsppaperwalk takes) walks some of them differently, so a walk with that step would fail here."""
    _, _, sc, tree, ref, _, bounds = walked
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


def test_device_entry_points_agree_with_the_host_ones(walked):
    _, _, sc, tree, _, oracle, bounds = walked
    twc.check_device_entry_points(sc, *_rays(tree, oracle, bounds, 4096, 3)[-4])      # the random rays


def test_quadric_variants_ran(quad):
    _, _, sc, tree, _, oracle, bounds = quad
    o, d, tm = _rays(tree, oracle, bounds, 4096, 5)[0]
    _, _, _, c = sc.intersect(o, d, tm, count=True)
    assert c[3] > 0      # sphere tests: the QUAD kernels walked


def test_bsppaperkd_renders_match_the_reference_images(hprt, bk):
    path, m, sc, _, _, _, _ = bk
    twc.check_reference_image(hprt, sc, m, path)


def test_counting_render_pixel_kd_stats(hprt, bk, tmp_path):
    _, m, sc, _, _, _, _ = bk
    st, px, check_plain_film = twc.check_counting_render(sc, m)
    kdc = sc.kd_counters()
    kd2 = sc.pixel_kd_stats()
    assert int(kd2[0].sum()) == kdc[0] and int(kd2[1].sum()) == kdc[1]
    assert (kd2[0] <= px[:, :, 5]).all() and (kd2[1] <= px[:, :, 6]).all()
    assert 0 < kdc[0] < st["nodes_entered"] and 0 < kdc[1] < st["nodes_entered_p"]      # kd nodes and plane nodes were both walked
    hprt.write_pixel_stats_rbspkd(str(tmp_path / "bk"), px, kd2)
    load = lambda n: np.loadtxt(tmp_path / ("bk-%s.txt" % n), dtype=np.uint64).reshape(px.shape[:2])
    assert np.array_equal(load("kdTreeNodeTraversals"), kd2[0]) and np.array_equal(load("kdTreeNodeTraversalsP"), kd2[1])
    assert np.array_equal(load("bspTreeNodeTraversals"), px[:, :, 5] - kd2[0])
    assert np.array_equal(load("bspTreeNodeTraversalsP"), px[:, :, 6] - kd2[1])
    check_plain_film()


def test_tile_sharded_render_merges_bit_identically(hprt, bk):
    _, m, sc, _, _, _, _ = bk
    twc.check_tile_sharding(hprt, sc, m)


def test_switching_among_the_bvh_and_all_five_trees_and_a_refused_attach(hprt):
    """BVH, then each of the five trees, then bsppaperkd again: each render is the one a scene with only that walk gives, with its
    counters and kd share; a refused attach leaves the walk before it in place."""
    m = hprt.Model.load(DODECA)
    opt = m.options.copy(); opt.spp = 2
    trees = {"bsppaperkd": ("attach_bsppaperkd", hprt.BspPaperKd(m)), "bsppaper": ("attach_bsppaper", hprt.BspPaper(m)),
             "rbspkd": ("attach_rbspkd", hprt.RbspKd(m, n_directions=7)), "rbsp": ("attach_rbsp", hprt.Rbsp(m, n_directions=7)),
             "kd": ("attach_kdtree", hprt.KdTree(m))}
    s = hprt.Scene(m, hprt.Bvh(m), device=0)
    alone = {"bvh": s.render(opt, count_work=True) + (s.kd_counters(),)}
    for name, (attach, tree) in trees.items():
        s = hprt.Scene(m, hprt.Bvh(m), device=0)
        getattr(s, attach)(tree)
        alone[name] = s.render(opt, count_work=True) + (s.kd_counters(),)
    assert alone["bsppaperkd"][2][0] > 0 and alone["bsppaper"][2] == (0, 0)
    sc = hprt.Scene(m, hprt.Bvh(m), device=0)
    bad = hprt.BspPaperKd.from_triangles(np.random.default_rng(0).uniform(0, 1, (7, 9)))      # not this scene's primitive count
    for name in ("bvh", "bsppaperkd", "bsppaper", "rbspkd", "bsppaperkd", "rbsp", "kd", "bsppaperkd"):
        if name != "bvh":
            getattr(sc, trees[name][0])(trees[name][1])
        for after in ("", " after a refused attach"):
            film, st = sc.render(opt, count_work=True)
            assert np.array_equal(film.view(np.uint32), alone[name][0].view(np.uint32)), name + after
            assert st["nodes_entered"] == alone[name][1]["nodes_entered"] and st["nodes_fetched"] == alone[name][1]["nodes_fetched"], name + after
            assert sc.kd_counters() == alone[name][2], name + after
            if not after:
                with pytest.raises(hprt.HprtError) as e:
                    sc.attach_bsppaperkd(bad)
                assert e.value.code == hprt.E_INVALID


def test_attach_refusals(hprt):
    mi = hprt.Model.load(os.path.join(GOLDEN, "simple_instanced.hprt"))
    si = hprt.Scene(mi, hprt.Bvh(mi), device=0)
    with pytest.raises(hprt.HprtError) as e:
        si.attach_bsppaperkd(hprt.BspPaperKd.from_triangles(np.random.default_rng(0).uniform(0, 1, (1, 9))))
    assert e.value.code == hprt.E_UNSUPPORTED
    with pytest.raises(hprt.HprtError) as e:
        hprt.BspPaperKd(mi)
    assert e.value.code == hprt.E_UNSUPPORTED
    m = hprt.Model.load(DODECA)
    sc = hprt.Scene(m, hprt.Bvh(m), device=0)
    opt = m.options.copy(); opt.spp = 1
    sc.render(opt)                                       # no kd-aware tree and no pixel statistics: nothing to read
    with pytest.raises(hprt.HprtError) as e:
        sc.pixel_kd_stats()
    assert e.value.code == hprt.E_INVALID


def test_example_attaches_the_bsppaperkd_tree(hprt, tmp_path):
    """examples/hprt_render.cpp on an Accelerator "bsppaperkd" scene: its image is Scene.attach_bsppaperkd + render's."""
    from test_kdtree_fallbacks import KD, _parse, _read_pfm
    exe = str(tmp_path / "hprt_render")
    lib = os.path.join(ROOT, "thesis-pbrt-v3_amd", "lib")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "hprt_render.cpp"), "-o", exe, "-L" + lib, "-lhprt", "-Wl,-rpath," + lib],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    m, path = _parse(hprt, tmp_path, KD.replace('Accelerator "kdtree"', 'Accelerator "bsppaperkd" "integer kdtraversalcost" [2]'), "bk.pbrt")
    out = str(tmp_path / "bk.pfm")
    r = subprocess.run([exe, path, out, "--spp", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert '"bvh" used' not in r.stderr and "hprt_scene_attach_bsppaperkd" in r.stderr, r.stderr
    opt = m.options.copy(); opt.spp = 2
    sc = hprt.Scene(m, hprt.Bvh(m), device=0)
    sc.attach_bsppaperkd(hprt.BspPaperKd(m))
    film, _ = sc.render(opt)
    assert np.array_equal(_read_pfm(out).view(np.uint32), hprt.film_resolve(film, opt.film_scale).view(np.uint32))


def test_bsppaperkd_walk_resources(hprt, tmp_path):
    """Triangle-only kernels: <= 80 registers (512 / 6 workgroups per CU), nothing in scratch; quadric kernels <= 128 (four); LDS:
    eight 8-byte todo entries per lane of a 256-thread workgroup."""
    twc.check_walk_resources(tmp_path, "k_bsppaperkdwalk", 8 * 256 * 8)
