"""Accelerator "bsppaper" on the host: the builder against the test-side restatement (tests/bsppaper_reference.cpp) node for node
(flags, split, axis) and in primitiveIndices, thread-count independence, a tree worked out by hand where a triangle's plane beats
every axis split, the planes of single triangles, the BVH classifications of the reference's own tests, the front end's
parameters and warnings, the refusals, the structural check behind attach and the pixel-statistics files.  No GPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, KILLEROO, ROOT
from tree_ref import bsppaper as bsppaper_ref

DODECA = os.path.join(GOLDEN, "dodecahedron.hprt")


def _f(u):
    return struct.unpack("<f", struct.pack("<I", int(u)))[0]


def _same_tree(hprt, p9, **kw):
    t = hprt.BspPaper.from_triangles(p9, **kw)
    nodes, idx = t.arrays()
    rn, ri = bsppaper_ref.build(p9, **kw)
    assert nodes.shape == rn.shape, (nodes.shape, rn.shape)
    interior = (nodes[:, 1] & 1) == 0
    assert np.array_equal(nodes[:, :2], rn[:, :2])
    assert np.array_equal(nodes[interior], rn[interior])          # the reference leaves a leaf's splitAxis unset
    assert not nodes[~interior, 2:].any()
    assert np.array_equal(idx, ri)
    return t, nodes, idx


def _soup(rng, n, grid=None, degenerate=0.0):
    c = rng.uniform(-10, 10, (n, 1, 3))
    e = rng.normal(0, 1.5, (n, 3, 3))
    p = (c + e).astype(np.float32)
    if grid:
        p = (np.round(p / grid) * grid).astype(np.float32)       # equal edge t values, coincident planes, axis-parallel edges
    k = rng.uniform(size=n) < degenerate
    p[k, 2] = p[k, 0]                                              # zero-area triangles: no planes
    return p.reshape(n, 9)


def test_dodecahedron_tree_equals_the_restatement(hprt):
    t = hprt.BspPaper(hprt.Model.load(DODECA))
    nodes, idx = t.arrays()
    rn, ri = bsppaper_ref.BspScene(DODECA).tree()
    interior = (nodes[:, 1] & 1) == 0
    assert np.array_equal(nodes[:, :2], rn[:, :2]) and np.array_equal(nodes[interior], rn[interior]) and np.array_equal(idx, ri)
    inf = t.info()
    assert inf["nodes"] == nodes.shape[0] and inf["prim_refs"] == idx.shape[0] and inf["leaves"] == int((~interior).sum())
    assert inf["axis_interior"] + inf["plane_interior"] == int(interior.sum()) and inf["plane_interior"] > 0


@pytest.mark.parametrize("seed", range(3))
@pytest.mark.parametrize("grid", [None, 0.5])
def test_random_soups_equal_the_restatement(hprt, seed, grid):
    rng = np.random.default_rng(100 + seed)
    _same_tree(hprt, _soup(rng, 150 + 50 * seed, grid=grid, degenerate=0.05))


def test_killeroo_prefix_equals_the_restatement(hprt):
    """a deterministic prefix of killeroo-simple's triangles (the restatement builds single-threaded)"""
    p9 = bsppaper_ref.BspScene(KILLEROO, build=False).triangles()
    assert p9.shape[0] > 50000
    _same_tree(hprt, p9[:1500])


@pytest.mark.parametrize("kw", [dict(max_prims=2), dict(empty_bonus=0.5), dict(trav_cost=1), dict(max_depth=4), dict(isect_cost=20, trav_cost=2)])
def test_non_default_parameters_equal_the_restatement(hprt, kw):
    _same_tree(hprt, _soup(np.random.default_rng(7), 200, grid=0.25), **kw)


def test_tree_is_independent_of_the_thread_count(hprt):
    p9 = _soup(np.random.default_rng(11), 1500)
    a = hprt.BspPaper.from_triangles(p9, threads=1).arrays()
    b = hprt.BspPaper.from_triangles(p9, threads=16).arrays()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_triangle_plane_split_by_hand(hprt):
    """Two triangles in z = 0 on either side of the diagonal x = y, a quarter off it: A (0.25, 0) (1, 0) (1, 0.75) below it,
    B (0, 0.25) (0.75, 1) (0, 1) above.  Their bounds overlap in x and in y, so every axis plane leaves one of them on both
    sides; the edge planes of their diagonal edges, axis PositiveX(Cross(n, p0 - p2)) = (1, -1, 0) / sqrt 2 and
    t = -+0.25 / sqrt 2, each cut one triangle off cleanly (the other touches the plane and goes to both sides), and the root's
    scan meets B's plane first.  Worked out (s = 1 / sqrt 2; a plane's above side is Dot(axis, p) >= t):
      0  plane (s, -s, 0), t = -0.25 s, above child 2
      1    leaf B                                        below: only B
      2    plane (s, -s, 0), t = +0.25 s, above child 8  above: A, and B, which touches the root plane
      3      plane x = 0.75, above child 7               below: B, and A, which touches this plane
      4        plane x = 0.25, above child 6             below x = 0.75: A and B
      5          leaf B                                  below x = 0.25: only B (A starts there)
      6          leaf A, B (primitiveIndices [1, 0])     above x = 0.25
      7        leaf A                                    above x = 0.75
      8    leaf A                                        above +0.25 s: only A"""
    A = np.array([[0.25, 0, 0], [1, 0, 0], [1, 0.75, 0]], np.float32)
    B = np.array([[0, 0.25, 0], [0.75, 1, 0], [0, 1, 0]], np.float32)
    p9 = np.stack([A, B]).reshape(2, 9)
    t, nodes, idx = _same_tree(hprt, p9)
    s = np.float32(1) / np.sqrt(np.float32(2))
    s = np.float32(1) / np.sqrt(s * s + s * s) * s                      # Normalize(Cross(...)) as the builder rounds it
    q = np.float32(0.25) * s
    d, x = [s, -s, 0], [1, 0, 0]
    I = lambda t_, above, ax: (np.float32(t_).view(np.uint32), above << 1, *np.array(ax, np.float32).view(np.uint32))
    L = lambda n, a: (a, 1 | n << 1, 0, 0, 0)
    want = np.array([I(-q, 2, d), L(1, 1), I(q, 8, d), I(0.75, 7, x), I(0.25, 6, x), L(1, 1), L(2, 0), L(1, 0), L(1, 0)], np.uint32)
    assert nodes[0, 1] == 4 and nodes[2, 1] == 16, nodes
    assert np.array_equal(nodes[:, 1], want[:, 1]) and np.array_equal(nodes[:, 2:], want[:, 2:]), (nodes, want)
    assert np.array_equal(nodes[[0, 2, 3, 4], 0].view(np.float32), want[[0, 2, 3, 4], 0].view(np.float32))
    assert nodes[1, 0] == 1 and nodes[5, 0] == 1 and nodes[7, 0] == 0 and nodes[8, 0] == 0
    assert list(idx) == [1, 0]
    assert t.info() == dict(nodes=9, leaves=5, depth=4, prim_refs=2, axis_interior=2, plane_interior=2)


def _lib_planes(hprt, tri9):
    import ctypes as C
    fn = hprt.lib.hprt_debug_bsppaper_planes
    fn.restype = C.c_int
    tri9 = np.ascontiguousarray(tri9, np.float32).reshape(9)
    out = np.zeros((4, 4), np.float32); k = C.c_uint32()
    assert fn(tri9.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.byref(k)) == 0
    return out[:k.value]


def _lib_classify(hprt, p9, plane4):
    import ctypes as C
    fn = hprt.lib.hprt_debug_bsppaper_classify
    fn.restype = C.c_int
    p9 = np.ascontiguousarray(p9, np.float32).reshape(-1, 9); plane4 = np.ascontiguousarray(plane4, np.float32)
    n = p9.shape[0]
    counts = np.zeros(2, np.uint32); left = np.zeros(2 * n, np.uint32); right = np.zeros(2 * n, np.uint32); sizes = np.zeros(2, np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert fn(C.c_size_t(n), vp(p9), vp(plane4), vp(counts), vp(left), vp(right), C.c_size_t(2 * n), vp(sizes)) == 0
    return (int(counts[0]), int(counts[1])), left[:sizes[0]], right[:sizes[1]]


@pytest.mark.parametrize("tri", [
    [[0, 0, 0], [1, 0, 0], [0, 1, 0]],                 # normal (0, 0, 1): x == 0 and y == 0 -> PositiveX gives (0, 0, 1)
    [[0, 0, 0], [0, 0, 1], [0, 1, 0]],                 # normal along -x -> flipped; axis-parallel edges
    [[0, 0, 0], [1, 0, 0], [0, 0, 1]],                 # normal (0, -1, 0): x == 0, y < 0 -> (0, 1, -0)
    [[0.5, -1, 2], [3, 0.25, -1], [-2, 1.5, 0.75]],    # generic
    [[1, 1, 1], [2, 2, 2], [3, 3, 3]],                 # collinear: no planes
    [[1, 2, 3], [1, 2, 3], [4, 5, 6]],                 # two equal vertices: no planes
])
def test_planes_of_single_triangles(hprt, tri):
    tri = np.array(tri, np.float32)
    got, want = _lib_planes(hprt, tri), bsppaper_ref.planes(tri)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)
    degenerate = np.linalg.norm(np.cross(tri[0] - tri[2], tri[1] - tri[2])) == 0
    assert (got.shape[0] == 0) == degenerate
    for p in got:
        assert p[1] > 0 or (p[1] == 0 and (p[2] > 0 or (p[2] == 0 and p[3] == 1)))    # PositiveX


def _tri(c, r=0.1):
    c = np.array(c, np.float32)
    return np.array([c + [-r, -r, 0], c + [r, -r, 0], c + [0, r, 0]], np.float32).reshape(9)


# The fork's own tests of the two classifications, tests/kdop.cpp TEST(BVH, amountLeftAndRight1..3) (:461-560): the triangles
# (0,0,0) (1,0,0) (1,1,0), then (3,3,3) (4,3,3) (4,4,3), then (1.5,3,3) (2.5,3,3) (2.5,4,3), against Plane(2, (1, 0, 0))
T0 = [0, 0, 0, 1, 0, 0, 1, 1, 0]
T1 = [3, 3, 3, 4, 3, 3, 4, 4, 3]
T2 = [1.5, 3, 3, 2.5, 3, 3, 2.5, 4, 3]
REF_BVH_CASES = [([T0], (1, 0), {0}, set()), ([T0, T1], (1, 1), {0}, {1}), ([T0, T1, T2], (2, 2), {0, 2}, {1, 2})]


@pytest.mark.parametrize("tris, counts, left, right", REF_BVH_CASES, ids=["amountLeftAndRight1", "amountLeftAndRight2", "amountLeftAndRight3"])
def test_bvh_classifications_of_the_reference_tests(hprt, tris, counts, left, right):
    p9 = np.array(tris, np.float32)
    plane4 = np.array([2, 1, 0, 0], np.float32)
    got = _lib_classify(hprt, p9, plane4)
    assert got[0] == counts
    assert len(got[1]) == len(left) and set(got[1].tolist()) == left          # (the reference asserts the lists as sets)
    assert len(got[2]) == len(right) and set(got[2].tolist()) == right
    want = bsppaper_ref.classify(p9, plane4)
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


def _tri(c, r=0.1):
    c = np.array(c, np.float32)
    return np.array([c + [-r, -r, 0], c + [r, -r, 0], c + [0, r, 0]], np.float32).reshape(9)


# further cases against the restatement: larger BVHs whose interior nodes lie wholly on one side, straddle or touch the plane
BVH_CASES = [
    ([_tri([-2, 0, 0]), _tri([-1, 0, 0]), _tri([1, 0, 0]), _tri([2, 0, 0])], [0, 1, 0, 0], (2, 2)),
    ([_tri([-2, 0, 0]), _tri([0, 0, 0]), _tri([2, 0, 0])], [0, 1, 0, 0], (2, 2)),
    ([_tri([x, y, 0]) for x in (-3, -1, 1, 3) for y in (-1, 1)], [1, 1, 0, 0], None),
    ([_tri([x, 0, 0], 0.6) for x in np.linspace(-2, 2, 9)], [0.25, 1, 0, 0], None),
]


@pytest.mark.parametrize("tris, plane, counts", BVH_CASES)
def test_bvh_classifications(hprt, tris, plane, counts):
    p9 = np.array(tris, np.float32)
    s = np.float32(1) / np.linalg.norm(np.array(plane[1:], np.float32)).astype(np.float32)
    plane4 = np.array([plane[0], plane[1] * s, plane[2] * s, plane[3] * s], np.float32)
    got = _lib_classify(hprt, p9, plane4)
    want = bsppaper_ref.classify(p9, plane4)
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    if counts is not None:
        assert got[0] == counts
    # every primitive lands on at least one side, a touching one on both
    assert set(got[1]) | set(got[2]) == set(range(p9.shape[0]))
    assert got[0] == (len(got[1]), len(got[2]))


def test_front_end_parameters_and_warnings(hprt, tmp_path):
    from test_host_side import _mesh_scene
    from test_kdtree_fallbacks import INSTANCED_KD
    P = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 1], [3, 0, 1], [2, 1, 1], [0, 2, 2], [1, 3, 2], [0, 3, 3]], np.float32)
    tri = np.arange(9, dtype=np.int32).reshape(3, 3)

    def parse(acc, text=None):
        p = tmp_path / "s.pbrt"
        p.write_text((text or _mesh_scene(P, tri)).replace('Accelerator "bvh"', acc).replace('Accelerator "kdtree"', acc))
        return hprt.Model.parse(str(p))

    m = parse('Accelerator "bsppaper"')
    assert m.accelerator == "bsppaper"
    assert any("hprt_scene_attach_bsppaper" in w for w in m.warnings())
    assert not any("outside the hot-path scope" in w for w in m.warnings())
    p9 = P[tri].reshape(-1, 9)
    assert np.array_equal(hprt.BspPaper(m).arrays()[0], hprt.BspPaper.from_triangles(p9).arrays()[0])
    m2 = parse('Accelerator "bsppaper" "integer nbDirections" [7] "integer maxprims" [2] "integer maxdepth" [3] "integer intersectcost" [20] '
               '"integer traversalcost" [2] "float emptybonus" [0.5]')
    assert not any("not used" in w for w in m2.warnings()), m2.warnings()
    assert np.array_equal(hprt.BspPaper(m2).arrays()[0], hprt.BspPaper.from_triangles(p9, 20, 2, 0.5, 2, 3).arrays()[0])
    m3 = parse('Accelerator "bsppaper" "integer bogus" [1]')
    assert any('"integer bogus" of Accelerator not used' in w for w in m3.warnings()), m3.warnings()
    # explicit parameters override the scene's line
    assert np.array_equal(hprt.BspPaper(m2, isect_cost=80).arrays()[0], hprt.BspPaper.from_triangles(p9).arrays()[0])
    # instanced scenes keep the BVH and the warning; the build is refused
    mi = parse('Accelerator "bsppaper"', INSTANCED_KD)
    assert any('"bsppaper" is outside the hot-path scope; "bvh" used' in w for w in mi.warnings())
    with pytest.raises(hprt.HprtError) as e:
        hprt.BspPaper(mi)
    assert e.value.code == hprt.E_UNSUPPORTED


CHECK_DRIVER = r"""
#include <cstdio>
#include <cstring>
#include "bsppaper_builder.h"
using namespace hprt;
static int fails = 0;
static void expect(const BspPaperTree &t, const char *want, uint32_t depth = 0) {
    uint32_t d = 12345;
    const char *got = CheckBspPaperTree(t, &d);
    if (std::strstr(got, want) == nullptr || (!*want && d != depth)) { std::printf("want '%s' got '%s' depth %u\n", want, got, d); ++fails; }
}
static BspNode leaf(uint32_t np, uint32_t a) { return BspNode{a, 1u | (np << 1)}; }
static BspNode interior(uint32_t above) { return BspNode{0x3f800000u, above << 1}; }
int main() {
    BspPaperTree t; t.nPrims = 3;
    t.nodes = {interior(2), leaf(1, 0), leaf(2, 0)}; t.primIndices = {1, 2}; t.axes = {0.6f, 0.8f, 0, 0, 0, 0, 0, 0, 0};
    expect(t, "", 1);
    BspPaperTree e = t; e.nodes.clear(); e.axes.clear(); expect(e, "no nodes");
    e = t; e.nodes[0] = interior(1); expect(e, "above child is out of range");
    e = t; e.nodes[1] = leaf(1, 3); expect(e, "one-primitive leaf");
    e = t; e.primIndices = {1, 7}; expect(e, "primitiveIndices names");
    e = t; e.axes.pop_back(); expect(e, "one axis per node");
    e = t; e.axes[0] = 0; e.axes[1] = 0; expect(e, "axis is zero");
    e = t; e.axes[1] = 1.f / 0.f; expect(e, "not finite");
    // a chain of 70 interior levels: the depth the attach step compares with the todo capacity (64)
    e = t; e.nodes.clear(); e.primIndices.clear(); e.axes.clear();
    for (uint32_t k = 0; k < 70; ++k) { e.nodes.push_back(interior(2 * k + 2)); e.nodes.push_back(leaf(0, 0)); }
    e.nodes.push_back(leaf(0, 0));
    for (size_t k = 0; k < e.nodes.size(); ++k) { e.axes.push_back(1); e.axes.push_back(0); e.axes.push_back(0); }
    expect(e, "", 70);
    return fails;
}
"""


def test_attach_check_rejects_malformed_trees(tmp_path):
    """CheckBspPaperTree (csrc/bsppaper_builder.cpp) is what hprt_scene_attach_bsppaper applies before anything reaches the device
    (and the depth it returns is held to HPRT_BSPPAPER_MAX_DEPTH); driven directly, built from the library's own source."""
    src = tmp_path / "check.cpp"
    src.write_text(CHECK_DRIVER)
    csrc = os.path.join(ROOT, "thesis-pbrt-v3_amd", "csrc")
    exe = str(tmp_path / "check")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-pthread", "-I" + csrc, str(src), os.path.join(csrc, "bsppaper_builder.cpp"),
                        os.path.join(csrc, "bvh_builder.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout


def test_pixel_stats_files_of_a_bsppaper_render(hprt, tmp_path):
    st = np.arange(3 * 4 * 7, dtype=np.uint64).reshape(3, 4, 7)
    assert hprt.ACCEL_BSP == hprt.ACCEL_RBSP
    hprt.write_pixel_stats_accel(str(tmp_path / "bp"), st, hprt.ACCEL_BSP)
    names = sorted(p.name for p in tmp_path.iterdir())
    assert names == sorted("bp-%s.txt" % n for n in ("primitiveIntersections", "primitiveIntersectionsP", "kdTreeNodeTraversals", "kdTreeNodeTraversalsP",
                                                   "bspTreeNodeTraversals", "bspTreeNodeTraversalsP", "leafNodeTraversals", "leafNodeTraversalsP"))
    assert np.array_equal(np.loadtxt(tmp_path / "bp-bspTreeNodeTraversals.txt", dtype=np.uint64), st[:, :, 5])
    assert np.array_equal(np.loadtxt(tmp_path / "bp-bspTreeNodeTraversalsP.txt", dtype=np.uint64), st[:, :, 6])
    assert np.loadtxt(tmp_path / "bp-kdTreeNodeTraversals.txt").sum() == 0
