"""Accelerator "bvhold" on the CPU: the library's stock BVH (hprt_bvhold_build / _from_bounds, csrc/bvhold_builder.cpp) equals the
test-side restatement (tests/bvhold_reference.cpp) bit for bit — bounds, offsets, counts, axes and the order — for the four split
methods; the HLBVH form's edge shapes, its order and its refusals; the front end; and the condition the GPU film test stands on.

The tie-free seeds.  tests/tree_fuzz.py's scenes random_scene(seed, objects=0, twins=False) at seeds 36 and 12 and objects=2 at
seeds 12 and 30 are the ones the issue names; test_the_restated_walk_finds_the_oracles_hits holds each of them, for "sah" and for
"hlbvh", to the oracle's t, primitive and barycentrics on all probe rays.  None had to be replaced."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import bvhold_cases as bc
import bvhold_ref
import tree_fuzz as tf
from conftest import GOLDEN, KILLEROO, ROOT
from tree_walk_checks import _bits

METHODS = ("sah", "hlbvh", "middle", "equal")
MAX_NODE_PRIMS = (1, 4, 255)
FILM_SEEDS = ((0, 36), (0, 12), (2, 12), (2, 30))      # (objects, seed); tests/test_gpu_bvhold.py renders exactly these


def _same(a, b, what):
    assert a[0].shape == b[0].shape and a[1].shape == b[1].shape, (what, a[0].shape, b[0].shape, a[1].shape, b[1].shape)
    assert np.array_equal(a[0], b[0]), (what, "nodes", int((a[0] != b[0]).any(1).argmax()))
    assert np.array_equal(a[1], b[1]), (what, "order")


def _well_formed(nodes, order, n):
    assert sorted(order.tolist()) == list(range(n))
    leaf = (nodes[:, 7] & 3) == 3
    assert int((nodes[leaf, 7] >> 2).sum()) == n and ((nodes[~leaf, 7] >> 2) == 0).all()      # an interior node's count is 0


@pytest.mark.parametrize("scene", ["dodecahedron.hprt", "killeroo_simple.hprt", "simple_instanced.hprt"])
@pytest.mark.parametrize("method", METHODS)
def test_scene_trees_equal_the_restatement(hprt, scene, method):
    path = os.path.join(GOLDEN, scene)
    m = hprt.Model.load(path)
    for mp in MAX_NODE_PRIMS:
        ref = bvhold_ref.BvhOldScene(path, method, mp)
        b = hprt.BvhOld(m, split_method=method, max_node_prims=mp)
        _same(b.arrays(), ref.tree(-1), (scene, method, mp, "top"))
        _well_formed(*b.arrays(), b.info()["prims"])
        for o in range(ref.n_objects):
            _same(b.object_arrays(o), ref.tree(o), (scene, method, mp, "object", o))
    if scene == "simple_instanced.hprt":
        assert ref.n_objects >= 1


@pytest.fixture(scope="module")
def killeroo_bounds():
    return bvhold_ref.BvhOldScene(KILLEROO, "equal", 4).bounds()


@pytest.mark.parametrize("method", METHODS)
def test_prefix_and_soups_equal_the_restatement(hprt, killeroo_bounds, method):
    lo, hi = killeroo_bounds
    sets = {"killeroo2000": (lo[:2000], hi[:2000])}
    for seed, n, scale in ((1, 3000, 1.0), (2, 1500, 0.05), (3, 800, 4.0)):      # three random soups: triangle bounds around random centres
        rng = np.random.default_rng(seed)
        P = (rng.uniform(-10, 10, (n, 1, 3)) + rng.normal(0, scale, (n, 3, 3))).astype(np.float32)
        sets["soup%d" % seed] = (P.min(1), P.max(1))
    for name, (bmin, bmax) in sets.items():
        for mp in MAX_NODE_PRIMS:
            b = hprt.BvhOld.from_bounds(bmin, bmax, method, mp)
            _same(b.arrays(), bvhold_ref.build(bmin, bmax, method, mp), (name, method, mp))
            _well_formed(*b.arrays(), bmin.shape[0])


SHAPES = bc.edge_shapes()


@pytest.mark.parametrize("name", list(SHAPES))
def test_hlbvh_edge_shapes(hprt, name):
    bmin, bmax, mp = SHAPES[name]
    n = bmin.shape[0]
    b = hprt.BvhOld.from_bounds(bmin, bmax, "hlbvh", mp)
    nodes, order = b.arrays()
    _same((nodes, order), bvhold_ref.build(bmin, bmax, "hlbvh", mp), name)
    _well_formed(nodes, order, n)
    # primOrder is the sorted Morton array: a stable sort of the codes
    codes = bc.morton_codes(bmin, bmax)
    assert np.array_equal(order, np.argsort(codes, kind="stable").astype(np.uint32)), name
    leaf = (nodes[:, 7] & 3) == 3
    counts = nodes[leaf, 7] >> 2
    if name in ("n1", "n2", "n3"):
        # n < maxnodeprims: every treelet's root is a leaf (the strict <), the upper SAH joins them
        treelets = len(np.unique(codes & 0x3ffc0000))
        assert leaf.sum() == treelets and nodes.shape[0] == 2 * treelets - 1
    if name == "n4":
        assert nodes.shape[0] > 1                                         # 4 < 4 is false
    if name == "all_equal":
        assert nodes.shape[0] == 1 and counts[0] == n
    if name == "flat_axis":
        assert len(np.unique(codes & 0x24924924)) == 1                    # no z bit is ever set
    if name == "lattice":
        assert counts.max() > mp and len(np.unique(codes)) <= 64          # bit-exhausted leaves larger than maxnodeprims
    if name == "offset_one":
        assert (codes == 0x3fffffff).sum() == 7                           # offset 1.0 on every axis: 1024 became 1023
    if name == "clamp":
        assert nodes.shape[0] == 5                                        # 300 clamps to 255: the treelet of 280 is split
        assert hprt.BvhOld.from_bounds(bmin, bmax, "hlbvh", 281).info()["nodes"] == 5


def test_empty_input_gives_an_empty_tree(hprt):
    for method in METHODS:
        b = hprt.BvhOld.from_bounds(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), method)
        assert b.info()["nodes"] == 0 and b.info()["prims"] == 0
        assert bvhold_ref.build(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), method)[0].shape[0] == 0


_HASH_SNIPPET = """
import hashlib, importlib, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import bvhold_cases as bc
hprt = importlib.import_module("thesis-pbrt-v3_amd")
bmin, bmax, mp = bc.edge_shapes()["n70001"]
for method in ("hlbvh", "sah"):
    nodes, order = hprt.BvhOld.from_bounds(bmin, bmax, method, mp).arrays()
    print(hashlib.sha256(nodes.tobytes() + order.tobytes()).hexdigest())
"""


def test_the_tree_does_not_depend_on_the_thread_count(hprt):
    bmin, bmax, mp = SHAPES["n70001"]
    want = []
    for method in ("hlbvh", "sah"):
        nodes, order = hprt.BvhOld.from_bounds(bmin, bmax, method, mp).arrays()
        want.append(hashlib.sha256(nodes.tobytes() + order.tobytes()).hexdigest())
    for threads in ("1", "7"):
        env = dict(os.environ, OMP_NUM_THREADS=threads)
        r = subprocess.run([sys.executable, "-c", _HASH_SNIPPET % (ROOT, os.path.join(ROOT, "tests"))], capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stderr
        assert r.stdout.split() == want, threads


def _refused(hprt, fn):
    with pytest.raises(hprt.HprtError) as e:
        fn()
    return e.value


def test_refusals(hprt):
    # a leaf of 65,536 primitives: a degenerate centroid extent (sah) and bit-exhausted codes (hlbvh)
    n = 65536
    c = np.tile([[1.0, 1.0, 1.0]], (n, 1)).astype(np.float32)
    h = (np.arange(n, dtype=np.float32).reshape(-1, 1) % 64 + 1) / 8
    for method in ("sah", "hlbvh"):
        e = _refused(hprt, lambda: hprt.BvhOld.from_bounds(c - h, c + h, method))
        assert e.code == hprt.E_UNSUPPORTED and "a leaf of 65536 primitives" in str(e) and "bvhOld.cpp:648" in str(e)
        with pytest.raises(RuntimeError):
            bvhold_ref.build(c - h, c + h, method)
        assert hprt.BvhOld.from_bounds((c - h)[:-1], (c + h)[:-1], method).info()["nodes"] == 1      # 65,535 are stored
    # more than 2^31 - 1 primitives: refused before anything is read
    one = np.zeros(3, np.float32)
    hnd = C.c_void_p()
    rc = hprt.lib.hprt_bvhold_build_from_bounds(2 ** 31, one.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p), None, C.byref(hnd))
    assert rc == hprt.E_UNSUPPORTED and "2^31 - 1" in hprt.lib.hprt_last_error().decode() and not hnd.value
    # the CHECK_NE of bvhOld.cpp:566, reached through the public entry with subnormal bounds: the primitives' centroids
    # .5f * pMin + .5f * pMax are 0 and 2^-149 (two treelets), the roots' (pMin + pMax) * .5f are 2^-149 both
    tiny = np.float32(2.0 ** -149)
    bmin = np.array([[tiny, 0, 0], [0, 0, 0]], np.float32); bmax = np.array([[tiny, 0, 0], [2 * tiny, 0, 0]], np.float32)
    assert bc.morton_codes(bmin, bmax).tolist() == [0, 0x9249249]
    e = _refused(hprt, lambda: hprt.BvhOld.from_bounds(bmin, bmax, "hlbvh", 1))
    assert e.code == hprt.E_UNSUPPORTED and "coincide on their widest axis" in str(e) and "bvhOld.cpp:566" in str(e)
    with pytest.raises(RuntimeError):
        bvhold_ref.build(bmin, bmax, "hlbvh", 1)
    # bounds whose sum overflows put a centroid outside the SAH buckets: the reference's CHECK_GE / CHECK_LT, refused and not indexed with
    big = np.array([[3e38, 0, 0], [2.9e38, 0, 0]], np.float32)
    e = _refused(hprt, lambda: hprt.BvhOld.from_bounds(big, big, "hlbvh", 1))
    assert e.code == hprt.E_UNSUPPORTED and "outside the 12 SAH buckets" in str(e)
    # bounds that are not finite: refused up front, whatever the method
    for bad in (np.nan, np.inf, -np.inf):
        lo, hi = bc.random_boxes(50, 9)
        hi[17, 1] = bad
        for method in METHODS:
            e = _refused(hprt, lambda: hprt.BvhOld.from_bounds(lo, hi, method))
            assert e.code == hprt.E_UNSUPPORTED and "the bounds of primitive 17 are not finite" in str(e)
    # finite bounds whose centroid extent overflows: the codes are formed without an undefined conversion (NaN offsets), and the
    # treelet roots' (pMin + pMax) overflows too, which the upper SAH refuses
    lo, hi = bc.huge_extent()
    e = _refused(hprt, lambda: hprt.BvhOld.from_bounds(lo, hi, "hlbvh", 4))
    assert e.code == hprt.E_UNSUPPORTED and "outside the 12 SAH buckets" in str(e)
    lo, hi = bc.huge_extent(flat=True)      # one treelet: every offset is 0 or NaN, every code 0, one leaf
    nodes, order = hprt.BvhOld.from_bounds(lo, hi, "hlbvh", 4).arrays()
    assert nodes.shape[0] == 1 and np.array_equal(order, np.arange(200, dtype=np.uint32))
    # an unknown split method
    prm = hprt.BvhOldParams(7, 4)
    rc = hprt.lib.hprt_bvhold_build_from_bounds(1, one.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p), C.byref(prm), C.byref(hnd))
    assert rc == hprt.E_INVALID and "split_method" in hprt.lib.hprt_last_error().decode()


def test_device_entries_refuse_without_a_device(hprt):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    bmin, bmax, mp = SHAPES["n64"]
    for method in ("hlbvh", "sah"):
        e = _refused(hprt, lambda: hprt.BvhOld.from_bounds(bmin, bmax, method, mp, device=0))
        assert e.code == hprt.E_NO_DEVICE and "no CPU fallback" in str(e)


SCENE = """LookAt 3 4 1.5  .5 .5 0  0 0 1
Camera "perspective" "float fov" [45]
Film "image" "integer xresolution" [32] "integer yresolution" [24]
Sampler "halton" "integer pixelsamples" [1]
Integrator "path" "integer maxdepth" [1]
Accelerator %s
WorldBegin
LightSource "point" "point from" [0 0 5] "color I" [10 10 10]
Shape "trianglemesh" "integer indices" [%s] "point P" [%s]
WorldEnd
"""
OLD_WARNING = '"bvh" used'
NEW_WARNING = ('Accelerator "bvhold": the host builds the tree (hprt_bvhold_build) and passes it to hprt_scene_create_from_model; '
               'hprt_bvh_build builds the fork\'s BVH')


def _parse(hprt, tmp_path, accel, name):
    rng = np.random.default_rng(5)
    n = 400
    P = (rng.uniform(-3, 3, (n, 1, 3)) + rng.normal(0, 0.2, (n, 3, 3))).astype(np.float32)
    p = tmp_path / (name + ".pbrt")
    p.write_text(SCENE % (accel, " ".join(str(i) for i in range(3 * n)), " ".join(repr(float(v)) for v in P.ravel())))
    return hprt.Model.parse(str(p)), P.min(1), P.max(1)


def test_front_end(hprt, tmp_path):
    trees = {}
    for method in METHODS:
        m, lo, hi = _parse(hprt, tmp_path, '"bvhold" "string splitmethod" "%s" "integer maxnodeprims" [2]' % method, method)
        assert m.accelerator == "bvhold"
        assert NEW_WARNING in m.warnings() and not any(OLD_WARNING in w for w in m.warnings()), m.warnings()
        assert not any("unknown" in w or "not used" in w or "unused" in w.lower() for w in m.warnings()), m.warnings()
        trees[method] = hprt.BvhOld(m).arrays()                      # params NULL: the Accelerator line's
        _same(trees[method], bvhold_ref.build(lo, hi, method, 2), method)
    assert len({t[0].tobytes() for t in trees.values()}) == 4        # four different trees: the names were told apart
    # the defaults: sah, 4
    m, lo, hi = _parse(hprt, tmp_path, '"bvhold"', "defaults")
    _same(hprt.BvhOld(m).arrays(), bvhold_ref.build(lo, hi, "sah", 4), "defaults")
    # an unknown method: the reference's warning, and sah
    m, lo, hi = _parse(hprt, tmp_path, '"bvhold" "string splitmethod" "best"', "unknown")
    assert 'BVH split method "best" unknown.  Using "sah".' in m.warnings() and NEW_WARNING in m.warnings()
    _same(hprt.BvhOld(m).arrays(), bvhold_ref.build(lo, hi, "sah", 4), "unknown")
    # maxnodeprims 300 clamps to 255
    m, lo, hi = _parse(hprt, tmp_path, '"bvhold" "string splitmethod" "hlbvh" "integer maxnodeprims" [300]', "clamp")
    _same(hprt.BvhOld(m).arrays(), bvhold_ref.build(lo, hi, "hlbvh", 255), "clamp")
    # hprt_bvh_build still builds the fork's BVH for a bvhold model, and a bvh model's warnings are what they were
    mb, _, _ = _parse(hprt, tmp_path, '"bvh"', "bvh")
    assert mb.accelerator == "bvh" and mb.warnings() == []
    m, _, _ = _parse(hprt, tmp_path, '"bvhold"', "defaults2")
    assert np.array_equal(hprt.Bvh(m).arrays()[0], hprt.Bvh(mb).arrays()[0])
    # every other name keeps its warning
    mk, _, _ = _parse(hprt, tmp_path, '"kdtreeold"', "kdtreeold")
    assert any('"kdtreeold" is outside the hot-path scope; "bvh" used' in w for w in mk.warnings())


def test_an_instanced_bvhold_model_gets_the_new_warning(hprt, tmp_path):
    text = tf.random_scene(12, objects=2, twins=False).replace("WorldBegin", 'Accelerator "bvhold" "string splitmethod" "hlbvh"\nWorldBegin', 1)
    assert "ObjectInstance" in text
    d = tmp_path
    from test_gpu_textures import _write_images
    _write_images(d)
    p = d / "inst.pbrt"
    p.write_text(text % {"dir": str(d)})
    m = hprt.Model.parse(str(p))
    assert NEW_WARNING in m.warnings() and not any(OLD_WARNING in w for w in m.warnings())
    path = str(d / "inst.hprt")
    m.save(path)
    ref = bvhold_ref.BvhOldScene(path, "hlbvh", 4)
    b = hprt.BvhOld(m)
    _same(b.arrays(), ref.tree(-1), "top")
    for o in range(ref.n_objects):
        _same(b.object_arrays(o), ref.tree(o), ("object", o))
    assert hprt.Model.load(path).accelerator == "bvh"      # the baked container does not change


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("bvhold_fuzz")


@pytest.mark.parametrize("objects,seed", FILM_SEEDS, ids=["o%d-s%d" % p for p in FILM_SEEDS])
def test_the_restated_walk_finds_the_oracles_hits(hprt, orc, workdir, objects, seed):
    """The tie-free condition the GPU film test stands on: on N_PROBE camera rays and N_PROBE random rays the restated bvhold walk
    finds the oracle's t, primitive, instance and barycentrics, for "sah" and for "hlbvh"."""
    text = tf.random_scene(seed, objects=objects, twins=False)
    m, path = tf.bake(hprt, workdir, text, "o%d_s%d" % (objects, seed))
    oracle = orc.OracleScene(path)
    fork = hprt.Bvh(m)
    rays = tf.joined(tf.probe_rays(m, oracle, fork.info()["bounds"], seed))
    t0, p0, i0, b0 = oracle.intersect_inst(*rays)[:4]
    n_obj = bvhold_ref.BvhOldScene(path, "equal", 4).n_objects
    c0 = bc.creation_ids(p0, [fork.arrays()[1]] + [fork.object_arrays(o)[1] for o in range(n_obj)])
    assert (p0 >= 0).sum() > 1000
    for method in ("sah", "hlbvh"):
        ref = bvhold_ref.BvhOldScene(path, method, 4)
        t1, p1, i1, b1, _ = ref.intersect(*rays)
        c1 = bc.creation_ids(p1, [ref.tree(-1)[1]] + [ref.tree(o)[1] for o in range(n_obj)])
        assert np.array_equal(c0, c1) and np.array_equal(i0, i1), (method, int((c0 != c1).sum()), int((i0 != i1).sum()))
        assert np.array_equal(_bits(t0), _bits(t1)) and np.array_equal(_bits(b0), _bits(b1)), method
