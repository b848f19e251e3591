"""The RBSP walk on the GPU (Accelerator "rbsp"): closest and any hit held bit for bit to the test-side restatement of
RBSP::Intersect / IntersectP (tests/rbsp_reference.cpp over tests/tree_reference.h) — t, primitive, barycentrics and all four
counters — on camera, random, degenerate, infinite and on-an-oblique-split-plane rays; renders against the reference's images;
per-pixel statistics; tile sharding; switching between the kd and RBSP walks; attach refusals; kernel resources.  The checks
shared with the other tree walks are tests/tree_walk_checks.py's."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, KILLEROO
from tree_ref import rbsp as rbsp_ref
import tree_walk_checks as twc

pytestmark = pytest.mark.gpu
DODECA = os.path.join(GOLDEN, "dodecahedron.hprt")
CASES = [(DODECA, 3), (DODECA, 7), (DODECA, 9), (DODECA, 13), (KILLEROO, 3), (KILLEROO, 7)]


@pytest.fixture(scope="module", params=CASES, ids=["dodecahedron-3", "dodecahedron-7", "dodecahedron-9", "dodecahedron-13", "killeroo-simple-3",
                                                   "killeroo-simple-7"])
def rb(request, hprt, orc):
    path, M = request.param
    m = hprt.Model.load(path)
    bvh = hprt.Bvh(m)
    sc = hprt.Scene(m, bvh, device=0)
    tree = hprt.Rbsp(m, n_directions=M)
    sc.attach_rbsp(tree)
    if path == DODECA:
        ref = rbsp_ref.RbspScene(path, M)                   # the restated build: the library's tree must be the same
        nodes, idx = tree.arrays()
        rn, ri = ref.tree()
        assert np.array_equal(nodes, rn) and np.array_equal(idx, ri)
    else:
        ref = rbsp_ref.RbspScene(path, M, build=False)     # killeroo-simple's restated build is slow: walk the library's tree
        ref.set_tree(*tree.arrays())
    b = np.array(bvh.info()["bounds"], np.float32)
    return path, M, m, sc, tree, ref, orc.OracleScene(path), (b[:3], b[3:])


def _rays(tree, ref, oracle, bounds, n, seed):
    rng = np.random.default_rng(seed)
    blo, bhi = bounds
    ext = bhi - blo
    # origins whose float Dot(dir, o) equals a split exactly (the belowFirst tie), oblique directions included
    ax, pos = ref.splits()
    return [twc.camera_rays(rng, oracle, n), twc.random_rays(rng, blo, ext, n), twc.degenerate_rays(rng, blo, ext, n),
            twc.plane_tie_rays(rng, blo, ext, n, tree.directions()[ax], pos)]


def test_closest_hit_equals_the_reference_walk(rb):
    _, _, _, sc, tree, ref, oracle, bounds = rb
    twc.check_closest(sc, ref, _rays(tree, ref, oracle, bounds, 20000, 1))


def test_any_hit_equals_the_reference_walk(rb):
    _, _, _, sc, tree, ref, oracle, bounds = rb
    twc.check_any(sc, ref, _rays(tree, ref, oracle, bounds, 20000, 2))


def test_device_entry_points_agree_with_the_host_ones(rb):
    _, _, _, sc, tree, ref, oracle, bounds = rb
    twc.check_device_entry_points(sc, *_rays(tree, ref, oracle, bounds, 4096, 3)[1])


def test_rbsp_renders_match_the_reference_images(hprt, rb):
    path, _, m, sc, _, _, _, _ = rb
    twc.check_reference_image(hprt, sc, m, path)


def test_counting_render_pixel_stats(hprt, rb, tmp_path):
    _, _, m, sc, _, _, _, _ = rb
    st, px, check_plain_film = twc.check_counting_render(sc, m)
    hprt.write_pixel_stats_accel(str(tmp_path / "rb"), px, hprt.ACCEL_RBSP)
    assert np.array_equal(np.loadtxt(tmp_path / "rb-bspTreeNodeTraversals.txt", dtype=np.uint64).reshape(px.shape[:2]), px[:, :, 5])
    assert np.array_equal(np.loadtxt(tmp_path / "rb-bspTreeNodeTraversalsP.txt", dtype=np.uint64).reshape(px.shape[:2]), px[:, :, 6])
    assert np.loadtxt(tmp_path / "rb-kdTreeNodeTraversals.txt").sum() == 0
    check_plain_film()


def test_tile_sharded_rbsp_render_merges_bit_identically(hprt, rb):
    _, _, m, sc, _, _, _, _ = rb
    twc.check_tile_sharding(hprt, sc, m)


def test_attaching_either_tree_replaces_the_other(hprt, orc):
    """rbsp after kd, then kd after rbsp: each render is the one a scene with only that tree gives, and the counters say
    which walk ran."""
    m = hprt.Model.load(DODECA)
    opt = m.options.copy(); opt.spp = 2
    kd, rbsp = hprt.KdTree(m), hprt.Rbsp(m, n_directions=7)
    alone = {}
    for name, attach, tree in (("kd", "attach_kdtree", kd), ("rbsp", "attach_rbsp", rbsp)):
        s = hprt.Scene(m, hprt.Bvh(m), device=0)
        getattr(s, attach)(tree)
        alone[name] = s.render(opt, count_work=True)
    assert alone["kd"][1]["nodes_entered"] != alone["rbsp"][1]["nodes_entered"]
    sc = hprt.Scene(m, hprt.Bvh(m), device=0)
    for name, attach, tree in (("kd", "attach_kdtree", kd), ("rbsp", "attach_rbsp", rbsp), ("kd", "attach_kdtree", kd)):
        getattr(sc, attach)(tree)
        film, st = sc.render(opt, count_work=True)
        assert np.array_equal(film.view(np.uint32), alone[name][0].view(np.uint32)), name
        assert st["nodes_entered"] == alone[name][1]["nodes_entered"] and st["nodes_fetched"] == alone[name][1]["nodes_fetched"], name


def test_attach_refusals(hprt):
    m = hprt.Model.load(DODECA)
    sc = hprt.Scene(m, hprt.Bvh(m), device=0)
    rng = np.random.default_rng(0)
    with pytest.raises(hprt.HprtError) as e:
        sc.attach_rbsp(hprt.Rbsp.from_triangles(rng.uniform(0, 1, (7, 9))))     # not this scene's primitive count
    assert e.value.code == hprt.E_INVALID
    mi = hprt.Model.load(os.path.join(GOLDEN, "simple_instanced.hprt"))
    si = hprt.Scene(mi, hprt.Bvh(mi), device=0)
    with pytest.raises(hprt.HprtError) as e:
        si.attach_rbsp(hprt.Rbsp.from_triangles(rng.uniform(0, 1, (1, 9))))
    assert e.value.code == hprt.E_UNSUPPORTED
    with pytest.raises(hprt.HprtError) as e:
        hprt.Rbsp(mi, n_directions=3)
    assert e.value.code == hprt.E_UNSUPPORTED
    # malformed child offsets, leaf ranges and depth are refused by CheckRbspTree (tests/test_rbsp_host.py drives every branch)


def test_rbsp_walk_resources(hprt, tmp_path):
    """Triangle-only kernels: <= 80 registers (six workgroups per CU), nothing in scratch; quadric kernels <= 128 (four);
    LDS: eight 8-byte todo entries per lane of a 256-thread workgroup plus the 13-direction table."""
    twc.check_walk_resources(tmp_path, "k_rbspwalk", 8 * 256 * 8 + 4 * 3 * 13)
