"""The node-based BSP trees on the GPU ("bspcluster", "bsprandomwithkd", "bsparbitraryfastkd", ...): they are walked by the kernels
that exist — a plain or withkd tree is a tree over BSPNode and takes k_bsppaperwalk, a fastkd tree a tree over BSPKdNode and takes
k_bsppaperkdwalk.  On each tree the device's closest and any hits equal the test-side restatement's walk (tests/bspnode_reference.cpp:
the restated build of the same seed must equal the library's, then BSP / BSPKd::Intersect and IntersectP) bit for bit — t,
primitive, barycentrics, all counters and for fastkd the kd share — on camera, random, degenerate, on-split-plane and
Dot(axis, d) == 0 rays.  The counting render, the reference image and tile sharding run on one tree of each node format; the C++
host example attaches a bspclusterfastkd tree.  Scenes: the dodecahedron, and killeroo-simple's first 2000 triangles with three
spheres (the QUAD kernels).  The checks are tests/tree_walk_checks.py's."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import bspnode_ref as nref
import tree_walk_checks as twc

pytestmark = pytest.mark.gpu
DODECA = os.path.join(GOLDEN, "dodecahedron.hprt")
K, SEED = 5, 7
TREES = [("dodecahedron", "bspcluster"), ("dodecahedron", "bsprandomwithkd"), ("dodecahedron", "bsparbitraryfastkd"),
         ("killeroo-prefix-spheres", "bspclusterfastkd"), ("killeroo-prefix-spheres", "bspcluster"), ("dodecahedron", "bsprandomfastkd")]
_SCENES, _PATHS = {}, {}


def _scene(key, hprt, orc, tmp_path_factory):
    """(path, model, scene with the attached tree, tree, restatement, oracle or None, BVH bounds), built once per module"""
    if key in _SCENES:
        return _SCENES[key]
    name, acc = key
    if name not in _PATHS:
        if name == "dodecahedron":
            _PATHS[name] = DODECA
        else:
            from test_gpu_bsppaper import _prefix_scene
            _PATHS[name] = _prefix_scene(tmp_path_factory, hprt)
    path = _PATHS[name]
    m = hprt.Model.load(path)
    bvh = hprt.Bvh(m)
    sc = hprt.Scene(m, bvh, device=0)
    tree, attach = hprt.bspnode_tree(m, acc, n_directions=K, seed=SEED)
    getattr(sc, attach)(tree)
    ref = nref.NodeScene(path, acc, K, SEED)              # the restated build: the library's tree must be the same
    nref.assert_same_tree(tree.arrays(), ref.tree(), acc.endswith("fastkd"))
    b = np.array(bvh.info()["bounds"], np.float32)
    _SCENES[key] = (path, m, sc, tree, ref, orc.OracleScene(path) if name == "dodecahedron" else None, (b[:3], b[3:]))
    return _SCENES[key]


@pytest.fixture(scope="module", params=TREES, ids=["%s-%s" % t for t in TREES])
def walked(request, hprt, orc, tmp_path_factory):
    return _scene(request.param, hprt, orc, tmp_path_factory) + (request.param[1],)


@pytest.fixture(scope="module", params=[TREES[1], TREES[5]], ids=["BSPNode", "BSPKdNode"])
def rendered(request, hprt, orc, tmp_path_factory):
    """One tree of each node format, on the scene with the reference's camera and image: the two with random directions.  The
    image check holds a render to the image of the reference's BVH, so it needs a tree that loses no hit, and the trees that split
    along primitive normals (arbitrary, cluster) do lose some — in the builder's own algorithm, not in the walk: a split plane
    then lies in a triangle's plane, and the sweep hands a triangle that starts and ends on the split to one child only.  The
    restated walk shows it on the CPU (DESIGN.md §8f has the ray); the device equals that walk on every tree above."""
    return _scene(request.param, hprt, orc, tmp_path_factory) + (request.param[1],)


def _split_planes(tree, fastkd):
    """(axes [P, 3], positions [P]) of the tree's interior nodes: the stored axis, or the unit axis of a fastkd tree's kd node"""
    nodes, _ = tree.arrays()
    if not fastkd:
        interior = (nodes[:, 1] & 1) == 0
        return nodes[interior, 2:].view(np.float32), nodes[interior, 0].view(np.float32)
    kind = nodes[:, 1] & nref.KIND_MASK
    kd, plane = kind < nref.LEAF, kind == nref.PLANE
    return (np.concatenate([np.eye(3, dtype=np.float32)[kind[kd]], nodes[plane, 2:].view(np.float32)]),
            np.concatenate([nodes[kd, 0].view(np.float32), nodes[plane, 0].view(np.float32)]))


def _rays(tree, fastkd, oracle, bounds, n, seed):
    rng = np.random.default_rng(seed)
    blo, bhi = bounds
    ext = bhi - blo
    out = [twc.camera_rays(rng, oracle, n)] if oracle is not None else []
    out += [twc.random_rays(rng, blo, ext, n), twc.degenerate_rays(rng, blo, ext, n)]
    # origins whose float Dot(axis, o) equals a node's split exactly (the belowFirst tie); a third of them with Dot(axis, d) == 0
    axes, pos = _split_planes(tree, fastkd)
    out.append(twc.plane_tie_rays(rng, blo, ext, n, axes, pos))
    return out


def test_walked_trees_hold_the_node_kinds_they_claim(walked):
    _, _, _, tree, _, _, _, acc = walked
    interior, axis = nref.interior_axes(tree.arrays()[0], acc.endswith("fastkd"))
    assert (interior & ~axis).sum() > 0
    if acc.endswith("kd"):
        assert axis.sum() > 0          # axis-aligned and oblique interior nodes are both walked


def test_closest_hit_equals_the_reference_walk(walked):
    _, _, sc, tree, ref, oracle, bounds, acc = walked
    twc.check_closest(sc, ref, _rays(tree, acc.endswith("fastkd"), oracle, bounds, 8192, 1))


def test_any_hit_equals_the_reference_walk(walked):
    _, _, sc, tree, ref, oracle, bounds, acc = walked
    twc.check_any(sc, ref, _rays(tree, acc.endswith("fastkd"), oracle, bounds, 8192, 2))


def test_quadric_variants_ran(hprt, orc, tmp_path_factory):
    for key in TREES[3:5]:
        _, _, sc, tree, _, _, bounds = _scene(key, hprt, orc, tmp_path_factory)
        o, d, tm = _rays(tree, key[1].endswith("fastkd"), None, bounds, 4096, 5)[0]
        _, _, _, c = sc.intersect(o, d, tm, count=True)
        assert c[3] > 0      # sphere tests: the QUAD kernels walked


def test_renders_match_the_reference_image(hprt, rendered):
    path, m, sc, _, _, _, _, _ = rendered
    twc.check_reference_image(hprt, sc, m, path)


def test_counting_render_and_pixel_statistics(hprt, rendered):
    _, m, sc, _, _, _, _, acc = rendered
    st, px, check_plain_film = twc.check_counting_render(sc, m)
    kdc = sc.kd_counters()
    if acc.endswith("fastkd"):
        kd2 = sc.pixel_kd_stats()
        assert int(kd2[0].sum()) == kdc[0] and int(kd2[1].sum()) == kdc[1]
        assert 0 < kdc[0] < st["nodes_entered"] and 0 < kdc[1] < st["nodes_entered_p"]      # kd nodes and plane nodes were both walked
    else:
        assert kdc == (0, 0)
    check_plain_film()


def test_tile_sharded_render_merges_bit_identically(hprt, rendered):
    _, m, sc, _, _, _, _, _ = rendered
    twc.check_tile_sharding(hprt, sc, m)


def test_example_attaches_the_bspclusterfastkd_tree(hprt, tmp_path):
    """examples/hprt_render.cpp on an Accelerator "bspclusterfastkd" scene: the tree is attached, not the BVH fallback, and its
    image is Scene.attach_bsppaperkd + render's."""
    from test_kdtree_fallbacks import KD, _parse, _read_pfm
    exe = str(tmp_path / "hprt_render")
    lib = os.path.join(ROOT, "thesis-pbrt-v3_amd", "lib")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "hprt_render.cpp"), "-o", exe, "-L" + lib, "-lhprt", "-Wl,-rpath," + lib],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    m, path = _parse(hprt, tmp_path, KD.replace('Accelerator "kdtree"', 'Accelerator "bspclusterfastkd" "integer nbDirections" [5] "integer seed" [3]'), "nb.pbrt")
    out = str(tmp_path / "nb.pfm")
    r = subprocess.run([exe, path, out, "--spp", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert '"bvh" used' not in r.stderr and "hprt_scene_attach_bsppaperkd" in r.stderr, r.stderr
    opt = m.options.copy(); opt.spp = 2
    sc = hprt.Scene(m, hprt.Bvh(m), device=0)
    tree = hprt.BspNodeKd(m)
    assert tree.info()["nodes"] > 1
    sc.attach_bsppaperkd(tree)
    film, _ = sc.render(opt)
    assert np.array_equal(_read_pfm(out).view(np.uint32), hprt.film_resolve(film, opt.film_scale).view(np.uint32))
