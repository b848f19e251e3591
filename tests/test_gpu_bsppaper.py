"""The general BSP walk on the GPU (Accelerator "bsppaper"): closest and any hit held bit for bit to the test-side restatement of
BSP::Intersect / IntersectP (tests/bsppaper_reference.cpp over tests/tree_reference.h) — t, primitive, barycentrics and all four
counters — on camera, random, degenerate, infinite and on-a-split-plane rays (the checks shared with the other tree walks are
tests/tree_walk_checks.py's); renders against the reference's image; per-pixel statistics; tile sharding;
switching between the BVH, bsppaper, RBSP and kd walks; attach refusals; kernel resources.  Scenes: the dodecahedron and a prefix
of killeroo-simple's triangles with three spheres (the restated build must equal the library's), and killeroo-simple (about 1.5
minutes to build on 16 threads; the restatement walks the library's tree)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from tree_ref import bsppaper as bsppaper_ref
import tree_walk_checks as twc

pytestmark = pytest.mark.gpu
DODECA = os.path.join(GOLDEN, "dodecahedron.hprt")
KILLEROO = os.path.join(GOLDEN, "killeroo_simple.hprt")


def _prefix_scene(tmp_path_factory, hprt):
    """killeroo-simple's first 2000 triangles and three spheres (one crossing the mesh), baked"""
    from test_host_side import HEADER
    p9 = bsppaper_ref.BspScene(KILLEROO, build=False).triangles()[:2000]
    P = p9.reshape(-1, 3)
    idx = np.arange(P.shape[0], dtype=np.int32)
    c = P.mean(0); r = float(np.abs(P - c).max())
    spheres = "".join('AttributeBegin Translate %r %r %r Shape "sphere" "float radius" [%r] AttributeEnd\n' % (float(x), float(y), float(z), rad)
                      for (x, y, z), rad in ((c, 0.2 * r), (c + [0.6 * r, 0, 0], 0.1 * r), (c - [0, 0.7 * r, 0.1 * r], 0.15 * r)))
    text = (HEADER + spheres + 'Shape "trianglemesh" "integer indices" [' + " ".join(map(str, idx)) + '] "point P" [' +
            " ".join(repr(float(v)) for v in P.ravel()) + "]\nWorldEnd\n")
    d = tmp_path_factory.mktemp("bsppaper")
    (d / "prefix.pbrt").write_text(text)
    m = hprt.Model.parse(str(d / "prefix.pbrt"))
    m.save(str(d / "prefix.hprt"))
    return str(d / "prefix.hprt")


_SCENES = {}


def _scene(name, hprt, orc, tmp_path_factory):
    """(path, model, scene with the attached bsppaper tree, tree, restatement, oracle or None, BVH bounds), built once per module"""
    if name in _SCENES:
        return _SCENES[name]
    path = {"dodecahedron": DODECA, "killeroo-simple": KILLEROO}.get(name) or _prefix_scene(tmp_path_factory, hprt)
    m = hprt.Model.load(path)
    bvh = hprt.Bvh(m)
    sc = hprt.Scene(m, bvh, device=0)
    tree = hprt.BspPaper(m)
    sc.attach_bsppaper(tree)
    nodes, idx = tree.arrays()
    if name != "killeroo-simple":
        ref = bsppaper_ref.BspScene(path)                 # the restated build: the library's tree must be the same
        rn, ri = ref.tree()
        interior = (nodes[:, 1] & 1) == 0
        assert np.array_equal(nodes[:, :2], rn[:, :2]) and np.array_equal(nodes[interior], rn[interior]) and np.array_equal(idx, ri)
    else:
        ref = bsppaper_ref.BspScene(path, build=False)    # killeroo-simple's restated build is slow: walk the library's tree
        ref.set_tree(nodes, idx)
    b = np.array(bvh.info()["bounds"], np.float32)
    _SCENES[name] = (path, m, sc, tree, ref, orc.OracleScene(path) if name != "killeroo-prefix-spheres" else None, (b[:3], b[3:]))
    return _SCENES[name]


@pytest.fixture(scope="module", params=["dodecahedron", "killeroo-simple", "killeroo-prefix-spheres"])
def walked(request, hprt, orc, tmp_path_factory):
    """the scenes the walks are held to the restatement on"""
    return _scene(request.param, hprt, orc, tmp_path_factory)


@pytest.fixture(scope="module", params=["dodecahedron", "killeroo-simple"])
def bp(request, hprt, orc, tmp_path_factory):
    """the scenes with the reference's camera and image"""
    return _scene(request.param, hprt, orc, tmp_path_factory)


@pytest.fixture(scope="module")
def quad(hprt, orc, tmp_path_factory):
    return _scene("killeroo-prefix-spheres", hprt, orc, tmp_path_factory)


def _rays(tree, oracle, bounds, n, seed):
    rng = np.random.default_rng(seed)
    blo, bhi = bounds
    ext = bhi - blo
    out = [twc.camera_rays(rng, oracle, n)] if oracle is not None else []
    out += [twc.random_rays(rng, blo, ext, n), twc.degenerate_rays(rng, blo, ext, n)]
    # origins whose float Dot(axis, o) equals a node's split exactly (the belowFirst tie), triangle planes included
    nodes, _ = tree.arrays()
    inner = (nodes[:, 1] & 1) == 0
    out.append(twc.plane_tie_rays(rng, blo, ext, n, nodes[inner, 2:].view(np.float32), nodes[inner, 0].view(np.float32)))
    return out


def test_closest_hit_equals_the_reference_walk(walked):
    _, _, sc, tree, ref, oracle, bounds = walked
    twc.check_closest(sc, ref, _rays(tree, oracle, bounds, 20000, 1))


def test_any_hit_equals_the_reference_walk(walked):
    _, _, sc, tree, ref, oracle, bounds = walked
    twc.check_any(sc, ref, _rays(tree, oracle, bounds, 20000, 2))


def test_quadric_variants_ran(quad):
    path, m, sc, tree, ref, oracle, bounds = quad
    o, d, tm = _rays(tree, oracle, bounds, 4096, 5)[0]
    _, _, _, c = sc.intersect(o, d, tm, count=True)
    assert c[3] > 0      # sphere tests: the QUAD kernels walked


def test_bsppaper_renders_match_the_reference_images(hprt, bp):
    path, m, sc, _, _, _, _ = bp
    twc.check_reference_image(hprt, sc, m, path)


def test_counting_render_pixel_stats(hprt, bp, tmp_path):
    path, m, sc, _, _, _, _ = bp
    st, px, check_plain_film = twc.check_counting_render(sc, m)
    hprt.write_pixel_stats_accel(str(tmp_path / "bp"), px, hprt.ACCEL_BSP)
    assert np.array_equal(np.loadtxt(tmp_path / "bp-bspTreeNodeTraversals.txt", dtype=np.uint64).reshape(px.shape[:2]), px[:, :, 5])
    check_plain_film()


def test_tile_sharded_render_merges_bit_identically(hprt, bp):
    path, m, sc, _, _, _, _ = bp
    twc.check_tile_sharding(hprt, sc, m)


def test_switching_walks_and_failed_attach(hprt):
    """BVH, then bsppaper, then rbsp, then kd: each render is the one a scene with only that walk gives; a refused attach leaves
    the walk before it in place."""
    m = hprt.Model.load(DODECA)
    opt = m.options.copy(); opt.spp = 2
    trees = {"bsppaper": ("attach_bsppaper", hprt.BspPaper(m)), "rbsp": ("attach_rbsp", hprt.Rbsp(m, n_directions=7)), "kd": ("attach_kdtree", hprt.KdTree(m))}
    alone = {"bvh": hprt.Scene(m, hprt.Bvh(m), device=0).render(opt, count_work=True)}
    for name, (attach, tree) in trees.items():
        s = hprt.Scene(m, hprt.Bvh(m), device=0)
        getattr(s, attach)(tree)
        alone[name] = s.render(opt, count_work=True)
    assert alone["bsppaper"][1]["nodes_entered"] != alone["rbsp"][1]["nodes_entered"]
    sc = hprt.Scene(m, hprt.Bvh(m), device=0)
    bad = hprt.BspPaper.from_triangles(np.random.default_rng(0).uniform(0, 1, (7, 9)))      # not this scene's primitive count
    for name in ("bvh", "bsppaper", "rbsp", "kd"):
        if name != "bvh":
            getattr(sc, trees[name][0])(trees[name][1])
        film, st = sc.render(opt, count_work=True)
        assert np.array_equal(film.view(np.uint32), alone[name][0].view(np.uint32)), name
        assert st["nodes_entered"] == alone[name][1]["nodes_entered"] and st["nodes_fetched"] == alone[name][1]["nodes_fetched"], name
        with pytest.raises(hprt.HprtError) as e:
            sc.attach_bsppaper(bad)
        assert e.value.code == hprt.E_INVALID
        film, st = sc.render(opt, count_work=True)
        assert np.array_equal(film.view(np.uint32), alone[name][0].view(np.uint32)), name + " after a refused attach"


def test_attach_refusals(hprt):
    mi = hprt.Model.load(os.path.join(GOLDEN, "simple_instanced.hprt"))
    si = hprt.Scene(mi, hprt.Bvh(mi), device=0)
    with pytest.raises(hprt.HprtError) as e:
        si.attach_bsppaper(hprt.BspPaper.from_triangles(np.random.default_rng(0).uniform(0, 1, (1, 9))))
    assert e.value.code == hprt.E_UNSUPPORTED
    with pytest.raises(hprt.HprtError) as e:
        hprt.BspPaper(mi)
    assert e.value.code == hprt.E_UNSUPPORTED


def test_bsppaper_walk_resources(hprt, tmp_path):
    """Triangle-only kernels: <= 80 registers (six workgroups per CU), nothing in scratch; quadric kernels <= 128 (four, as the
    RBSP walk's); LDS: eight 8-byte todo entries per lane of a 256-thread workgroup."""
    twc.check_walk_resources(tmp_path, "k_bsppaperwalk", 8 * 256 * 8)
