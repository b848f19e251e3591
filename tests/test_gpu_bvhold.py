"""Accelerator "bvhold" on the GPU.  The device build of the HLBVH form (csrc/device/hlbvh_build.hip) gives the host build's tree
byte for byte — on the edge shapes of tests/bvhold_cases.py, around the sort's tiles, on equal codes across workgroups, on scenes
with and without instances and with both emit paths on one input.  A scene created from a bvhold tree is walked by the existing
kernels (k_walk4, the binary walk, occlusion, the two-level walk) to the restatement's hits and counts; a leaf of 300 triangles
too.  On the tie-free seeds of tests/test_bvhold_host.py the film through a bvhold tree is the film through the fork's BVH, plain,
counting and with per-pixel statistics, and those statistics are the restatement's counts on the camera rays."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bvhold_cases as bc
import bvhold_ref
import tree_fuzz as tf
import tree_walk_checks as twc
from conftest import GOLDEN, KILLEROO, ROOT
from test_bvhold_host import FILM_SEEDS
from tree_walk_checks import _bits

gpu = pytest.mark.gpu
SHAPES = dict(bc.edge_shapes(), **bc.sort_shapes())
UNIT = os.path.join(ROOT, "thesis-pbrt-v3_amd", "csrc", "device", "hlbvh_build.hip")
KERNELS = ("k_hlbvh_centroids", "k_hlbvh_morton", "k_radix_hist", "k_radix_scan", "k_radix_scatter", "k_hlbvh_treelets", "k_hlbvh_compact",
           "k_hlbvh_emit", "k_hlbvh_pack")


def _same(a, b, what):
    assert a[0].shape == b[0].shape and a[1].shape == b[1].shape, (what, a[0].shape, b[0].shape)
    assert np.array_equal(a[1], b[1]), (what, "order", int((a[1] != b[1]).argmax()))
    assert np.array_equal(a[0], b[0]), (what, "nodes", int((a[0] != b[0]).any(1).argmax()))


def _treelet_sizes(bmin, bmax):
    keys = np.sort(bc.morton_codes(bmin, bmax) >> 18)
    return np.unique(keys, return_counts=True)[1]


@gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_device_build_equals_host_build(hprt, name):
    bmin, bmax, mp = SHAPES[name]
    host = hprt.BvhOld.from_bounds(bmin, bmax, "hlbvh", mp)
    dev = hprt.BvhOld.from_bounds(bmin, bmax, "hlbvh", mp, device=0)
    _same(dev.arrays(), host.arrays(), name)
    assert dev.info() == host.info()
    sizes = _treelet_sizes(bmin, bmax)
    st = dev.build_stats
    assert st["prims_sorted"] == bmin.shape[0] and st["sort_passes"] == 4 and st["treelets"] == len(sizes), st
    assert st["treelets_host"] == int((sizes > 4096).sum()), st
    # centroids, codes, 4 x (histogram, scan, scatter), treelet marks, compaction, emit; the pack when a treelet came from the device
    assert st["launches"] == 2 + 12 + 3 + (1 if (sizes <= 4096).any() else 0), st
    if name == "equal_codes":
        assert np.array_equal(dev.arrays()[1], np.arange(8192, dtype=np.uint32))      # stability: equal keys keep their order


@gpu
@pytest.mark.parametrize("name", ["n4097", "lattice", "n70001", "tile8193"])
def test_both_emit_paths_on_one_input(hprt, name):
    """serial_treelet_max 16: treelets of more primitives are emitted on the host from the downloaded sorted array"""
    bmin, bmax, mp = SHAPES[name]
    host = hprt.BvhOld.from_bounds(bmin, bmax, "hlbvh", mp)
    dev = hprt.BvhOld.from_bounds(bmin, bmax, "hlbvh", mp, device=0, serial_treelet_max=16)
    _same(dev.arrays(), host.arrays(), name)
    sizes = _treelet_sizes(bmin, bmax)
    assert dev.build_stats["treelets_host"] == int((sizes > 16).sum()) and dev.build_stats["treelets"] == len(sizes)
    if name == "n70001":
        assert 0 < dev.build_stats["treelets_host"] < len(sizes)      # both paths ran (about 17 primitives per treelet)
    if name == "lattice":
        assert dev.build_stats["treelets_host"] == len(sizes)         # about 78 per treelet: all on the host


@gpu
@pytest.mark.parametrize("scene", ["killeroo_simple.hprt", "simple_instanced.hprt"])
def test_device_build_of_a_model(hprt, scene):
    m = hprt.Model.load(os.path.join(GOLDEN, scene))
    host = hprt.BvhOld(m, split_method="hlbvh")
    for smax in (0, 16):
        dev = hprt.BvhOld(m, split_method="hlbvh", device=0, serial_treelet_max=smax)
        _same(dev.arrays(), host.arrays(), (scene, "top"))
        n_obj = bvhold_ref.BvhOldScene(os.path.join(GOLDEN, scene), "equal", 4).n_objects
        prims = host.info()["prims"]
        for o in range(n_obj):
            _same(dev.object_arrays(o), host.object_arrays(o), (scene, "object", o))
            prims += host.object_arrays(o)[1].shape[0]
        assert dev.build_stats["prims_sorted"] == prims      # every tree went through the one session
    assert (n_obj > 0) == (scene == "simple_instanced.hprt")


@gpu
def test_refusals_of_the_device_entries(hprt):
    bmin, bmax, mp = SHAPES["n64"]
    for method in ("sah", "middle", "equal"):
        with pytest.raises(hprt.HprtError) as e:
            hprt.BvhOld.from_bounds(bmin, bmax, method, mp, device=0)
        assert e.value.code == hprt.E_UNSUPPORTED and "hprt_bvhold_build builds" in str(e.value)
    with pytest.raises(hprt.HprtError) as e:
        hprt.BvhOld.from_bounds(bmin, bmax, "hlbvh", mp, device=0, serial_treelet_max=65537)
    assert e.value.code == hprt.E_INVALID and "serial_treelet_max may only lower" in str(e.value)
    with pytest.raises(hprt.HprtError) as e:
        hprt.BvhOld.from_bounds(bmin, bmax, "hlbvh", mp, device=1000)
    assert e.value.code == hprt.E_INVALID and "ordinal" in str(e.value)
    # what the host entries refuse up front the device entries refuse alike: bounds that are not finite
    bad = bmax.copy(); bad[5, 2] = np.nan
    with pytest.raises(hprt.HprtError) as e:
        hprt.BvhOld.from_bounds(bmin, bad, "hlbvh", mp, device=0)
    assert e.value.code == hprt.E_UNSUPPORTED and "the bounds of primitive 5 are not finite" in str(e.value)
    # finite bounds whose centroid extent overflows (NaN offsets): the device forms the host's codes, and the upper SAH's refusal is the host's
    lo, hi = bc.huge_extent()
    msgs = []
    for device in (None, 0):
        with pytest.raises(hprt.HprtError) as e:
            hprt.BvhOld.from_bounds(lo, hi, "hlbvh", 4, device=device)
        assert e.value.code == hprt.E_UNSUPPORTED
        msgs.append(str(e.value))
    assert msgs[0] == msgs[1] and "outside the 12 SAH buckets" in msgs[0]
    lo, hi = bc.huge_extent(flat=True)      # every offset 0 or NaN: every code 0 on the device as on the host, one leaf
    host = hprt.BvhOld.from_bounds(lo, hi, "hlbvh", 4).arrays()
    _same(hprt.BvhOld.from_bounds(lo, hi, "hlbvh", 4, device=0).arrays(), host, "huge extent")
    assert host[0].shape[0] == 1
    # the host build's refusal comes back from the device build: a leaf of 65,536 primitives
    c = np.ones((65536, 3), np.float32)
    with pytest.raises(hprt.HprtError) as e:
        hprt.BvhOld.from_bounds(c - 0.5, c + 0.5, "hlbvh", 4, device=0, serial_treelet_max=65536)
    assert e.value.code == hprt.E_UNSUPPORTED and "a leaf of 65536 primitives" in str(e.value)


class _Walked:
    """a scene created from a bvhold tree, its restatement and probe rays"""

    def __init__(self, hprt, orc, path, method, device):
        self.model = hprt.Model.load(path)
        self.bvh = hprt.BvhOld(self.model, split_method=method, device=device)
        self.scene = hprt.Scene(self.model, self.bvh)
        self.ref = bvhold_ref.BvhOldScene(path, method, 4)
        _same(self.bvh.arrays(), self.ref.tree(-1), (path, method))
        oracle = orc.OracleScene(path)
        rng = np.random.default_rng(11)
        b = np.array(self.bvh.info()["bounds"], np.float32)
        n = 20000
        self.rays = tf.joined([twc.camera_rays(rng, oracle, n), twc.random_rays(rng, b[:3], b[3:] - b[:3], n)])


def _check_walks(hprt, w, instanced):
    """t, primitive, instance, barycentrics and occlusion per ray; the counters (count=True) as the entry points give them: totals
    over all rays, held to the sums of the restatement's per-ray counts"""
    o, d, tm = w.rays
    t0, p0, i0, b0, c0 = w.ref.intersect(o, d, tm)
    occ0, q0 = w.ref.occluded(o, d, tm)
    assert 0.02 < (p0 >= 0).mean() < 0.98 and 0.02 < occ0.mean() < 0.98
    sc = w.scene
    hprt.lib.hprt_debug_wide_walk.argtypes = [C.c_int]
    try:
        for wide in (1, 0):      # k_walk4, then the binary walk
            hprt.lib.hprt_debug_wide_walk(wide)
            t1, p1, i1, b1 = sc.intersect_instanced(o, d, tm)
            assert np.array_equal(p0, p1) and np.array_equal(i0, i1), (wide, int((p0 != p1).sum()), int((i0 != i1).sum()))
            assert np.array_equal(_bits(t0), _bits(t1)) and np.array_equal(_bits(b0), _bits(b1)), wide
            assert np.array_equal(occ0, sc.occluded(o, d, tm)), wide
            if not instanced:
                t2, p2, b2 = sc.intersect(o, d, tm)
                assert np.array_equal(p0, p2) and np.array_equal(_bits(t0), _bits(t2)) and np.array_equal(_bits(b0), _bits(b2)), wide
    finally:
        hprt.lib.hprt_debug_wide_walk(-1)
    # counting: nodes fetched, nodes entered, triangle and sphere tests are the restatement's
    t3, p3, i3, b3, c3 = sc.intersect_instanced(o, d, tm, count=True)
    assert np.array_equal(p0, p3) and np.array_equal(_bits(t0), _bits(t3))
    assert c3.tolist() == c0[:, :4].sum(0).tolist(), (c3, c0.sum(0))
    occ3, q3 = sc.occluded(o, d, tm, count=True)
    assert np.array_equal(occ0, occ3) and q3.tolist() == q0[:, :4].sum(0).tolist(), (q3, q0.sum(0))
    assert (i0 >= 0).any() == instanced


@gpu
@pytest.mark.parametrize("method,device", [("sah", None), ("hlbvh", 0)])
def test_walks_of_a_bvhold_scene_equal_the_restatement(hprt, orc, method, device):
    _check_walks(hprt, _Walked(hprt, orc, KILLEROO, method, device), False)


@gpu
@pytest.mark.parametrize("method,device", [("sah", None), ("hlbvh", 0)])
def test_walks_of_an_instanced_bvhold_scene_equal_the_restatement(hprt, orc, method, device):
    _check_walks(hprt, _Walked(hprt, orc, os.path.join(GOLDEN, "simple_instanced.hprt"), method, device), True)


LEAF_SCENE = """LookAt 0 -5 0  0 0 0  0 0 1
Camera "perspective" "float fov" [45]
Film "image" "integer xresolution" [32] "integer yresolution" [32]
Sampler "halton" "integer pixelsamples" [1]
Integrator "path" "integer maxdepth" [1]
WorldBegin
LightSource "point" "point from" [0 -4 3] "color I" [10 10 10]
Shape "trianglemesh" "integer indices" [%s] "point P" [%s]
WorldEnd
"""


@gpu
def test_a_leaf_of_300_triangles_is_walked(hprt, tmp_path):
    """every box has the same centre: the builds make one leaf of 300 primitives, which the layout marks by its last primitive"""
    ks = np.linspace(-0.99, 0.99, 300).astype(np.float32)
    P = np.concatenate([np.array([[-1, -1, -1], [1, 1, 1], [1, -1, k]], np.float32) for k in ks])
    p = tmp_path / "leaf.pbrt"
    p.write_text(LEAF_SCENE % (" ".join(str(i) for i in range(900)), " ".join(repr(float(v)) for v in P.ravel())))
    m = hprt.Model.parse(str(p))
    path = str(tmp_path / "leaf.hprt")
    m.save(path)
    rng = np.random.default_rng(3)
    o, d, tm = twc.random_rays(rng, np.full(3, -1, np.float32), np.full(3, 2, np.float32), 4096)
    for method, device in (("sah", None), ("hlbvh", 0)):
        b = hprt.BvhOld(m, split_method=method, device=device)
        nodes, order = b.arrays()
        assert nodes.shape[0] == 1 and nodes[0, 7] == (3 | (300 << 2))
        ref = bvhold_ref.BvhOldScene(path, method, 4)
        _same((nodes, order), ref.tree(-1), method)
        sc = hprt.Scene(m, b)
        t0, p0, i0, b0, c0 = ref.intersect(o, d, tm)
        t1, p1, b1, c1 = sc.intersect(o, d, tm, count=True)
        assert np.array_equal(p0, p1) and np.array_equal(_bits(t0), _bits(t1)) and np.array_equal(_bits(b0), _bits(b1))
        assert c1.tolist() == c0[:, :4].sum(0).tolist() and (p0 >= 0).sum() > 100 and c1[2] >= 300
        t2, p2, b2 = sc.intersect(o, d, tm)
        assert np.array_equal(p0, p2) and np.array_equal(_bits(t0), _bits(t2))
        occ0, _ = ref.occluded(o, d, tm)
        assert np.array_equal(occ0, sc.occluded(o, d, tm))


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("bvhold_films")


@gpu
@pytest.mark.parametrize("objects,seed", FILM_SEEDS, ids=["o%d-s%d" % p for p in FILM_SEEDS])
def test_film_through_a_bvhold_tree_is_the_forks(hprt, orc, workdir, objects, seed):
    m, path = tf.bake(hprt, workdir, tf.random_scene(seed, objects=objects, twins=False), "o%d_s%d" % (objects, seed))
    film0, st0 = hprt.Scene(m, hprt.Bvh(m)).render()
    assert film0[..., :3].max() > 0 and st0["shadow_rays"] > 0
    oracle = orc.OracleScene(path)
    x0, y0, x1, y1 = m.options.film_bounds()
    py, px = np.mgrid[y0:y1, x0:x1]
    oc, dc = oracle.camera_rays(px.ravel().astype(np.int32), py.ravel().astype(np.int32), np.zeros(px.size, np.int64))
    for method, device in (("sah", None), ("hlbvh", 0)):
        what = "%s, o%d s%d" % (method, objects, seed)
        sc = hprt.Scene(m, hprt.BvhOld(m, split_method=method, device=device))
        plain, st = sc.render()
        assert np.array_equal(plain.view(np.uint32), film0.view(np.uint32)), what
        counted, stc = sc.render(count_work=True)
        assert np.array_equal(counted.view(np.uint32), film0.view(np.uint32)), what + " (counting)"
        stats_film, stp = sc.render(pixel_stats=True)
        assert np.array_equal(stats_film.view(np.uint32), film0.view(np.uint32)), what + " (pixel statistics)"
        assert (stp["camera_rays"], stp["rays"], stp["shadow_rays"]) == (stc["camera_rays"], stc["rays"], stc["shadow_rays"])
        # the statistics themselves, on camera rays alone (one sample, no bounce): the restatement's counts over THIS tree
        opt = m.options.copy()
        opt.spp = 1; opt.max_depth = 0
        sc.render(opt, pixel_stats=True)
        px7 = sc.pixel_stats().reshape(-1, 7)
        c = bvhold_ref.BvhOldScene(path, method, 4).intersect(oc, dc, np.full(oc.shape[0], np.inf, np.float32))[4]
        assert (px7[:, 0] == 1).all(), what
        assert np.array_equal(px7[:, 1], c[:, 2] + c[:, 3]), what + ": primitiveIntersections"
        assert np.array_equal(px7[:, 3], c[:, 4]), what + ": leafNodeTraversals"
        assert np.array_equal(px7[:, 5], c[:, 1] - c[:, 4]), what + ": bvhTreeNodeTraversals"
        assert px7[:, 1].sum() > 0 and px7[:, 5].sum() > 0


def test_the_new_units_kernels_use_no_scratch_and_the_lds_they_state(hprt, tmp_path):
    """from the code object's metadata (no GPU needed): no kernel of device/hlbvh_build.hip has scratch or spills a VGPR, and its
    LDS per workgroup is what the unit's static_assert states"""
    stated = {}
    for value, names in re.findall(r'static_assert\(kLds\w+ == (\d+), "LDS ([\w ]+)"\);', open(UNIT).read()):
        for k in names.split():
            stated[k] = int(value)
    ks = twc.kernel_metadata(twc.LIBHPRT, tmp_path)
    for kernel in KERNELS:
        found = [v for n, v in ks.items() if kernel in n]
        assert len(found) == 1, kernel
        k = found[0]
        assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, kernel
        assert k[".group_segment_fixed_size"] == stated.get(kernel, 0), (kernel, k[".group_segment_fixed_size"])
        assert k[".wavefront_size"] == 64 and k[".max_flat_workgroup_size"] == (64 if kernel == "k_hlbvh_emit" else 256), kernel
    assert set(stated) == {"k_hlbvh_centroids", "k_radix_hist", "k_radix_scan", "k_hlbvh_compact", "k_radix_scatter", "k_hlbvh_emit"}


@gpu
def test_builds_in_turn_then_a_render_with_the_stock_tree(hprt, killeroo_model):
    """three device builds in turn, a refused one in the middle; then the fork's BVH renders its golden image as before"""
    bmin, bmax, mp = SHAPES["n4097"]
    host = hprt.BvhOld.from_bounds(bmin, bmax, "hlbvh", mp).arrays()
    _same(hprt.BvhOld.from_bounds(bmin, bmax, "hlbvh", mp, device=0).arrays(), host, "first")
    with pytest.raises(hprt.HprtError) as e:
        hprt.BvhOld.from_bounds(bmin, bmax, "sah", mp, device=0)
    assert e.value.code == hprt.E_UNSUPPORTED
    _same(hprt.BvhOld.from_bounds(bmin, bmax, "hlbvh", mp, device=0).arrays(), host, "third")
    sc = hprt.Scene(killeroo_model, hprt.Bvh(killeroo_model))
    twc.check_reference_image(hprt, sc, killeroo_model, KILLEROO)
