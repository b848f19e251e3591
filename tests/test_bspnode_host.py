"""The node-based BSP accelerators on the host ("bsparbitrary", "bspcluster", "bsprandom" and their "withkd" / "fastkd" forms): the
builder against the test-side restatement (tests/bspnode_reference.cpp, given the same seed) node for node — flags, splits, the
axes of the nodes that have one, primitiveIndices — for all nine names; seeds and thread counts; the direction choosers on their
own; a scene whose choice is known; the refusals; the front end; bsppaper and bsppaperkd trees unchanged.  The reference seeds from
std::random_device and cannot be reproduced: parity is unpinned.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, KILLEROO, ROOT
from tree_ref import bsppaper as bsppaper_ref
import bsppaperkd_ref
import bspnode_ref as nref
from test_bsppaper_host import _soup

DODECA = os.path.join(GOLDEN, "dodecahedron.hprt")
KS = (4, 6)


def _lib_tree(hprt, p9, acc, **kw):
    fast = acc.endswith("fastkd")
    if not fast:
        kw.pop("kd_trav_cost", None)
    return (hprt.BspNodeKd if fast else hprt.BspNode).from_triangles(p9, acc, **kw)


def _same_tree(hprt, p9, acc, both_kinds=True, **kw):
    """the library's tree over p9 is the restatement's; a withkd / fastkd tree holds axis-aligned and oblique interior nodes"""
    fast = acc.endswith("fastkd")
    t = _lib_tree(hprt, p9, acc, **kw)
    nodes, idx = t.arrays()
    nref.assert_same_tree((nodes, idx), nref.build(p9, acc, **kw), fast)
    interior, axis = nref.interior_axes(nodes, fast)
    inf = t.info()
    assert (inf["nodes"], inf["prim_refs"], inf["leaves"]) == (nodes.shape[0], idx.shape[0], int((~interior).sum()))
    if fast:
        assert not nodes[(nodes[:, 1] & 7) != nref.PLANE, 2:].any()       # kd nodes and leaves: the axis words are written as zero
        assert (inf["kd_interior"], inf["plane_interior"]) == (int(axis.sum()), int((interior & ~axis).sum()))
    else:
        assert not nodes[~interior, 2:].any()
    if acc.endswith("kd"):
        assert inf["kd_interior" if fast else "axis_interior"] == int(axis.sum())
        if both_kinds:
            assert axis.sum() > 0 and (interior & ~axis).sum() > 0, (int(axis.sum()), int(interior.sum()))
    return t, nodes, idx


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("acc", nref.ACCELERATORS)
def test_dodecahedron_tree_equals_the_restatement(hprt, acc, K):
    fast = acc.endswith("fastkd")
    m = hprt.Model.load(DODECA)
    t, attach = hprt.bspnode_tree(m, acc, n_directions=K, seed=3)
    assert attach == ("attach_bsppaperkd" if fast else "attach_bsppaper")
    nodes, idx = t.arrays()
    nref.assert_same_tree((nodes, idx), nref.NodeScene(DODECA, acc, K, 3).tree(), fast)
    interior, axis = nref.interior_axes(nodes, fast)
    if acc.endswith("kd"):
        assert axis.sum() > 0 and (interior & ~axis).sum() > 0


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("acc", nref.ACCELERATORS)
def test_soups_equal_the_restatement(hprt, acc, K):
    """three soups of at most 300 triangles: random, grid-snapped (equal edge values, axis-parallel normals) and one with zero-area
    triangles (whose normal is (0, 0, 0): PositiveX makes it (0, 0, 1))"""
    for seed, (n, grid, degenerate) in enumerate(((150, None, 0.05), (200, 0.5, 0.0), (300, 0.25, 0.05))):
        _same_tree(hprt, _soup(np.random.default_rng(100 + seed), n, grid=grid, degenerate=degenerate), acc, n_directions=K, seed=11 + seed)


@pytest.fixture(scope="module")
def killeroo_prefix():
    p9 = bsppaper_ref.BspScene(KILLEROO, build=False).triangles()
    assert p9.shape[0] > 50000
    return p9[:2000]


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("acc", nref.ACCELERATORS)
def test_killeroo_prefix_equals_the_restatement(hprt, killeroo_prefix, acc, K):
    _same_tree(hprt, killeroo_prefix, acc, n_directions=K)        # the default seed


@pytest.mark.parametrize("kw", [dict(trav_cost=1), dict(trav_cost=40, kd_trav_cost=5), dict(kd_trav_cost=20), dict(max_prims=2), dict(max_depth=4),
                                dict(empty_bonus=0.5), dict(isect_cost=20, trav_cost=2, kd_trav_cost=2), dict(n_directions=3), dict(n_directions=9)])
@pytest.mark.parametrize("acc", ["bspcluster", "bsparbitrarywithkd", "bsprandomfastkd"])
def test_non_default_parameters_equal_the_restatement(hprt, acc, kw):
    kw = dict(dict(n_directions=5, seed=2), **kw)
    _same_tree(hprt, _soup(np.random.default_rng(7), 200, grid=0.25), acc, both_kinds=False, **kw)


# ---- seeds and threads ----

@pytest.mark.parametrize("acc", ["bsparbitrary", "bspclusterwithkd", "bsprandomfastkd"])
def test_seeds(hprt, acc):
    p9 = _soup(np.random.default_rng(21), 250)
    a, b, c = (_lib_tree(hprt, p9, acc, n_directions=5, seed=s).arrays() for s in (1, 1, 2))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])                   # the same seed: the same tree
    assert a[0].shape != c[0].shape or not np.array_equal(a[0], c[0])                 # another seed: another tree
    d = _lib_tree(hprt, p9, acc, n_directions=5).arrays()                              # no seed: the documented default
    e = _lib_tree(hprt, p9, acc, n_directions=5, seed=5489).arrays()
    assert hprt.BSPNODE_DEFAULT_SEED == 5489 and np.array_equal(d[0], e[0]) and np.array_equal(d[1], e[1])


@pytest.mark.parametrize("acc", ["bspcluster", "bsprandomwithkd", "bsparbitraryfastkd"])
def test_tree_is_independent_of_the_thread_count(hprt, acc):
    p9 = _soup(np.random.default_rng(11), 1500)           # 3000 edges per direction: well past the 1024 candidates that go to threads
    a = _lib_tree(hprt, p9, acc, n_directions=5, seed=9, threads=1).arrays()
    b = _lib_tree(hprt, p9, acc, n_directions=5, seed=9, threads=16).arrays()
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ---- the choosers on their own ----

def _lib_choose(hprt, chooser, K, seed, p9, draws=1):
    fn = hprt.lib.hprt_debug_bspnode_choose
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    p9 = np.ascontiguousarray(p9, np.float32).reshape(-1, 9)
    counts = np.zeros(draws, np.uint32); dirs = np.zeros((draws * max(K, p9.shape[0]), 3), np.float32)
    rc = fn(nref.CHOOSERS.index(chooser), K, seed, p9.shape[0], p9.ctypes.data, draws, counts.ctypes.data, dirs.ctypes.data)
    assert rc == 0, rc
    ends = np.cumsum(counts)
    return [dirs[e - c:e].copy() for c, e in zip(counts, ends)]


def _same_draws(hprt, chooser, K, seed, p9, draws):
    got, want = _lib_choose(hprt, chooser, K, seed, p9, draws), nref.choose(chooser, K, seed, p9, draws)
    assert len(got) == len(want) == draws
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.tobytes() == w.tobytes()
    return got


def _normals(hprt, p9):
    """PositiveX(Normal()) of each triangle: what the arbitrary chooser returns for K >= np (every index drawn, in set order)"""
    return _lib_choose(hprt, "arbitrary", p9.shape[0], 1, p9)[0]


def test_drawn_index_sets(hprt):
    """chooseArbitraryNormals returns the normals of the drawn indices in std::set order: with distinct normals the rows name the
    index set, which must be the restatement's random_int draws (a double in [0, np) truncated to uint32_t)"""
    p9 = _soup(np.random.default_rng(31), 40)
    normals = _normals(hprt, p9)
    assert np.unique(normals, axis=0).shape[0] == 40
    for seed in range(5):
        ids = nref.draw_ids(6, 40, seed, draws=3)
        assert (np.diff(ids.astype(np.int64), axis=1) > 0).all() and ids.max() < 40
        for g, row in zip(_same_draws(hprt, "arbitrary", 6, seed, p9, 3), ids):
            assert g.tobytes() == normals[row].tobytes()


def test_random_directions(hprt):
    for seed in range(4):
        for g in _same_draws(hprt, "random", 7, seed, _soup(np.random.default_rng(1), 3), 3):
            assert g.shape == (7, 3) and (g[:, 0] >= 0).all()
            assert np.allclose(np.linalg.norm(g.astype(np.float64), axis=1), 1, atol=1e-6)


def test_cluster_means(hprt):
    p9 = _soup(np.random.default_rng(41), 120, grid=0.5, degenerate=0.1)
    for seed in range(4):
        for K in (1, 2, 5):
            for g in _same_draws(hprt, "cluster", K, seed, p9, 2):
                assert g.shape == (K, 3)


def test_cluster_redraws_when_a_cluster_is_empty(hprt):
    """Every triangle has the same normal, so the two first means are equal, every normal goes to cluster 0 (ties keep the first
    mean) and cluster 1 is empty: the means are drawn again, 500 times over.  The second call from the same engine only agrees with
    the restatement if each of those draws was taken."""
    p9 = _soup(np.random.default_rng(43), 30)
    p9 = p9.reshape(30, 3, 3).copy(); p9[:, :, 2] = 0; p9 = p9.reshape(30, 9)       # all in z = 0: PositiveX normal (0, 0, 1)
    for seed in range(3):
        got = _same_draws(hprt, "cluster", 2, seed, p9, 2)
        assert all(np.array_equal(g, [[0, 0, 1], [0, 0, 1]]) for g in got)


def test_np_at_most_K_shortcut(hprt):
    """calculateClusterMeans returns the node's normals undrawn for np <= K, chooseArbitraryNormals draws min(np, K) indices"""
    p9 = _soup(np.random.default_rng(51), 4)
    normals = _normals(hprt, p9)
    for K in (4, 6):
        g = _same_draws(hprt, "cluster", K, 5, p9, 2)
        assert all(x.tobytes() == normals.tobytes() for x in g)
        g = _same_draws(hprt, "arbitrary", K, 5, p9, 2)
        assert all(x.tobytes() == normals.tobytes() for x in g)
    assert _same_draws(hprt, "cluster", 3, 5, p9, 1)[0].shape == (3, 3)


# ---- a scene whose choice is known ----

def _two_orientation_scene():
    """twelve triangles of two orientations: six in planes z = const (PositiveX normal (0, 0, 1)) and six in planes x + y = const
    (PositiveX normal (1, 1, 0) / sqrt 2), spread so that both kinds of plane separate primitives"""
    A = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)            # exact translates: each orientation's normals are bit-equal
    B = np.array([[1, 0, 0.25], [0, 1, 0.25], [1, 0, 1]], np.float32)
    tris = []
    for k in range(6):
        tris.append(A + np.float32([k, 0, k]))
        tris.append(B + np.float32([2 * k, 0, k]))
    return np.array(tris, np.float32).reshape(-1, 9)


def test_bspcluster_splits_only_along_the_two_orientations(hprt):
    """bspcluster at K = 2 over a scene with exactly two normal orientations: k-means settles on the two (a cluster of equal unit
    vectors has their direction as its mean, to the rounding of Normalize(n * v)), or — below the root, where a node may hold one
    orientation only, or two primitives — returns the normals themselves; so every interior axis is one of the two."""
    p9 = _two_orientation_scene()
    normals = _normals(hprt, p9)
    two = np.unique(normals, axis=0)
    assert two.shape == (2, 3) and np.array_equal(two[0], [0, 0, 1]) and two[1, 2] == 0 and two[1, 0] == two[1, 1] > 0.7
    for seed in range(6):
        _, nodes, _ = _same_tree(hprt, p9, "bspcluster", n_directions=2, seed=seed)
        interior = (nodes[:, 1] & 1) == 0
        assert interior.sum() >= 3
        axes = nodes[interior, 2:].view(np.float32)
        near = np.abs(axes[:, None, :] - two[None]).max(2) <= 1e-6
        assert near.any(1).all(), axes[~near.any(1)]
        assert near[:, 0].any() and near[:, 1].any()              # both orientations split somewhere


# ---- refusals ----

@pytest.mark.parametrize("acc", [a for a in nref.ACCELERATORS if a.endswith("kd")])
def test_fewer_than_three_directions_is_refused(hprt, acc):
    p9 = _soup(np.random.default_rng(3), 20)
    for K in (0, 1, 2):
        with pytest.raises(hprt.HprtError) as e:
            _lib_tree(hprt, p9, acc, n_directions=K)
        assert e.value.code == hprt.E_UNSUPPORTED and "nbDirections" in str(e.value)
        with pytest.raises(RuntimeError):
            nref.build(p9, acc, n_directions=K)
    _same_tree(hprt, p9, acc, both_kinds=False, n_directions=3)    # K = 3: the axes alone, nothing drawn


def test_plain_forms_take_small_K(hprt):
    p9 = _soup(np.random.default_rng(3), 20)
    for acc in ("bsparbitrary", "bspcluster", "bsprandom"):
        _same_tree(hprt, p9, acc, n_directions=1, seed=4)
    with pytest.raises(hprt.HprtError) as e:                       # k-means over no means reads means[0]
        _lib_tree(hprt, p9, "bspcluster", n_directions=0)
    assert e.value.code == hprt.E_UNSUPPORTED


def test_instanced_models_and_wrong_builders_are_refused(hprt):
    mi = hprt.Model.load(os.path.join(GOLDEN, "simple_instanced.hprt"))
    for cls, acc in ((hprt.BspNode, "bspcluster"), (hprt.BspNodeKd, "bspclusterfastkd")):
        with pytest.raises(hprt.HprtError) as e:
            cls(mi, acc)
        assert e.value.code == hprt.E_UNSUPPORTED and "instances" in str(e.value)
    with pytest.raises(ValueError):
        hprt.BspNode.from_triangles(_soup(np.random.default_rng(3), 5), "bspclusterfastkd")
    with pytest.raises(ValueError):
        hprt.BspNodeKd.from_triangles(_soup(np.random.default_rng(3), 5), "bspcluster")
    m = hprt.Model.load(DODECA)                                    # a baked model's accelerator is "bvh": params are needed
    with pytest.raises(hprt.HprtError) as e:
        hprt.BspNode(m)
    assert e.value.code == hprt.E_INVALID


def _check(hprt, nodes, idx, n_prims, kd_aware):
    fn = hprt.lib.hprt_debug_bspnode_check
    fn.restype = C.c_int
    fn.argtypes = [C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p]
    nodes = np.ascontiguousarray(nodes, np.uint32); idx = np.ascontiguousarray(idx, np.uint32)
    depth = C.c_uint32(0)
    rc = fn(nodes.shape[0], nodes.ctypes.data, idx.shape[0], idx.ctypes.data, n_prims, 1 if kd_aware else 0, C.byref(depth))
    return rc, depth.value


@pytest.mark.parametrize("kd_aware", [False, True])
def test_trees_deeper_than_64_levels_are_refused(hprt, kd_aware):
    """the structural check behind the builds and the attach, driven directly: a well-formed chain of interior nodes, each with an
    empty leaf below it, is accepted at 64 levels (the walks' todo capacity) and refused as unsupported at 65"""
    one = np.float32(1).view(np.uint32)
    shift, leaf, plane = (3, 3, 4) if kd_aware else (1, 1, 0)

    def chain(levels):
        rows = []
        for k in range(levels):
            rows.append([one, plane | ((2 * k + 2) << shift), one, 0, 0])     # split 1.0 along (1, 0, 0); above child two on
            rows.append([0, leaf, 0, 0, 0])
        rows.append([0, leaf, 0, 0, 0])
        return np.array(rows, np.uint32)

    assert _check(hprt, chain(64), np.zeros(0, np.uint32), 0, kd_aware) == (0, 64)
    rc, depth = _check(hprt, chain(65), np.zeros(0, np.uint32), 0, kd_aware)
    assert rc == hprt.E_UNSUPPORTED and depth == 65
    bad = chain(3); bad[0, 1] = plane | (99 << shift)
    assert _check(hprt, bad, np.zeros(0, np.uint32), 0, kd_aware)[0] == hprt.E_INVALID
    header = open(os.path.join(ROOT, "include", "hprt.h")).read()
    assert "#define HPRT_BSPPAPER_MAX_DEPTH 64" in header and "#define HPRT_BSPPAPERKD_MAX_DEPTH 64" in header


# ---- the front end (fails on the parent: the nine names fell back to the BVH with a warning) ----

@pytest.mark.parametrize("acc", nref.ACCELERATORS)
def test_front_end_parameters_and_warnings(hprt, tmp_path, acc):
    from test_host_side import _mesh_scene
    from test_kdtree_fallbacks import INSTANCED_KD
    fast = acc.endswith("fastkd")
    rng = np.random.default_rng(5)
    P = (rng.uniform(-4, 4, (12, 1, 3)) + rng.normal(0, 1, (12, 3, 3))).astype(np.float32).reshape(-1, 3)
    tri = np.arange(36, dtype=np.int32).reshape(12, 3)
    p9 = P[tri].reshape(-1, 9)
    cls = hprt.BspNodeKd if fast else hprt.BspNode
    build, attach = ("hprt_bspnodekd_build", "hprt_scene_attach_bsppaperkd") if fast else ("hprt_bspnode_build", "hprt_scene_attach_bsppaper")

    def parse(line, text=None):
        p = tmp_path / "s.pbrt"
        p.write_text((text or _mesh_scene(P, tri)).replace('Accelerator "bvh"', line).replace('Accelerator "kdtree"', line))
        return hprt.Model.parse(str(p))

    m = parse('Accelerator "%s"' % acc)
    assert m.accelerator == acc
    assert any(build + ")" in w and attach in w for w in m.warnings()), m.warnings()
    assert not any("outside the hot-path scope" in w or "not used" in w for w in m.warnings()), m.warnings()
    same = lambda a, b: np.array_equal(a.arrays()[0], b.arrays()[0]) and np.array_equal(a.arrays()[1], b.arrays()[1])
    assert same(cls(m), _lib_tree(hprt, p9, acc))                                            # the defaults: K = 3, the default seed
    t, how = hprt.bspnode_tree(m)
    assert how == "attach_bsppaperkd" if fast else how == "attach_bsppaper"
    assert same(t, cls(m))
    kdline = ' "integer kdtraversalcost" [4]' if fast else ""
    m2 = parse('Accelerator "%s" "integer nbDirections" [6] "integer seed" [77] "integer maxprims" [2] "integer maxdepth" [5] "integer intersectcost" [20] '
               '"integer traversalcost" [2] "float emptybonus" [0.5]%s' % (acc, kdline))
    assert not any("not used" in w for w in m2.warnings()), m2.warnings()
    kw = dict(n_directions=6, seed=77, max_prims=2, max_depth=5, isect_cost=20, trav_cost=2, empty_bonus=0.5, kd_trav_cost=4)
    assert same(cls(m2), _lib_tree(hprt, p9, acc, **kw))
    nref.assert_same_tree(cls(m2).arrays(), nref.build(p9, acc, **kw), fast)
    assert same(cls(m2, acc), _lib_tree(hprt, p9, acc))                                      # explicit parameters override the scene's line
    m3 = parse('Accelerator "%s" "integer bogus" [1]' % acc)
    assert any('"integer bogus" of Accelerator not used' in w for w in m3.warnings()), m3.warnings()
    if not fast:                                                                             # "kdtraversalcost" belongs to the fastkd forms
        m4 = parse('Accelerator "%s" "integer kdtraversalcost" [4]' % acc)
        assert any('"integer kdtraversalcost" of Accelerator not used' in w for w in m4.warnings()), m4.warnings()
    mi = parse('Accelerator "%s"' % acc, INSTANCED_KD)                                       # instanced: the BVH and the warning stay
    assert any('"%s" is outside the hot-path scope; "bvh" used' % acc in w for w in mi.warnings()), mi.warnings()
    assert not any(attach in w for w in mi.warnings())
    with pytest.raises(hprt.HprtError) as e:
        cls(mi)
    assert e.value.code == hprt.E_UNSUPPORTED


def test_seed_belongs_to_the_node_based_names_only(hprt, tmp_path):
    from test_host_side import _mesh_scene
    P = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 1], [3, 0, 1], [2, 1, 1]], np.float32)
    tri = np.arange(6, dtype=np.int32).reshape(2, 3)
    for acc in ("bvh", "kdtree", "rbsp", "bsppaper", "bsppaperkd"):
        p = tmp_path / "s.pbrt"
        p.write_text(_mesh_scene(P, tri).replace('Accelerator "bvh"', 'Accelerator "%s" "integer seed" [3]' % acc))
        assert any('"integer seed" of Accelerator not used' in w for w in hprt.Model.parse(str(p)).warnings()), acc


# ---- the existing trees ----

def test_bsppaper_and_bsppaperkd_trees_are_unchanged(hprt):
    """their builder now takes its helpers from csrc/bsp_build.h: the trees are still the existing restatements'"""
    m = hprt.Model.load(DODECA)
    nodes, idx = hprt.BspPaper(m).arrays()
    rn, ri = bsppaper_ref.BspScene(DODECA).tree()
    interior = (nodes[:, 1] & 1) == 0
    assert np.array_equal(nodes[:, :2], rn[:, :2]) and np.array_equal(nodes[interior], rn[interior]) and np.array_equal(idx, ri)
    bsppaperkd_ref.assert_same_tree(hprt.BspPaperKd(m).arrays(), bsppaperkd_ref.BspKdScene(DODECA).tree())
    p9 = _soup(np.random.default_rng(301), 200, grid=0.5)
    nodes, idx = hprt.BspPaper.from_triangles(p9).arrays()
    rn, ri = bsppaper_ref.build(p9)
    interior = (nodes[:, 1] & 1) == 0
    assert np.array_equal(nodes[:, :2], rn[:, :2]) and np.array_equal(nodes[interior], rn[interior]) and np.array_equal(idx, ri)
    bsppaperkd_ref.assert_same_tree(hprt.BspPaperKd.from_triangles(p9).arrays(), bsppaperkd_ref.build(p9))
