"""Accelerator "rbsp" on the host: the builder against the test-side restatement (tests/rbsp_reference.cpp) node for node, the
direction table, thread-count independence, a tree worked out by hand, structural invariants, the front end's parameters and
warnings, the refusals, the structural check behind attach and the fork's pixel-statistics files for an RBSP render.  No GPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, KILLEROO, ROOT
from tree_ref import rbsp as rbsp_ref

DODECA = os.path.join(GOLDEN, "dodecahedron.hprt")


def _f2u(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def _off(M):
    return 32 - (M.bit_length() and (32 - M.bit_length()))      # 32 - clz(M)


def _same_tree(hprt, p9, M, **kw):
    t = hprt.Rbsp.from_triangles(p9, M, **kw)
    nodes, idx = t.arrays()
    rn, ri, rd = rbsp_ref.build(p9, M, **kw)
    assert nodes.shape == rn.shape and np.array_equal(nodes, rn), (nodes.shape, rn.shape)
    assert np.array_equal(idx, ri)
    assert np.array_equal(t.directions().view(np.uint32), rd.view(np.uint32))
    return t, nodes, idx


def test_direction_table_is_the_reference_formula(hprt):
    """getDirections (accelerators/RBSPShared.h): the axes, then (M 7, 13) the four diagonals, then (M 9, 13) the six face
    diagonals, each Normalize(v) = v * (1 / sqrt(x*x + y*y + z*z)) in float."""
    def nz(v):
        v = np.array(v, np.float32)
        ln = np.sqrt(np.float32(v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]).astype(np.float32)
        return v * (np.float32(1) / ln)
    axes = [np.array(a, np.float32) for a in ([1, 0, 0], [0, 1, 0], [0, 0, 1])]
    diag = [nz(v) for v in ([1, 1, 1], [1, -1, 1], [1, 1, -1], [1, -1, -1])]
    face = [nz(v) for v in ([1, 1, 0], [1, 0, 1], [0, 1, 1], [1, -1, 0], [1, 0, -1], [0, 1, -1])]
    tri = np.zeros((1, 9), np.float32)
    tri[0, 3:6] = 1
    for M, want in ((3, axes), (7, axes + diag), (9, axes + face), (13, axes + diag + face)):
        got = hprt.Rbsp.from_triangles(tri, M).directions()
        assert np.array_equal(got.view(np.uint32), np.array(want, np.float32).view(np.uint32)), M
        assert hprt.Rbsp.from_triangles(tri, M).info()["M"] == M


@pytest.mark.parametrize("M", [3, 7, 9, 13])
def test_dodecahedron_trees_equal_the_restatement(hprt, M):
    m = hprt.Model.load(DODECA)
    t = hprt.Rbsp(m, n_directions=M)
    nodes, idx = t.arrays()
    rn, ri = rbsp_ref.RbspScene(DODECA, M).tree()
    assert np.array_equal(nodes, rn) and np.array_equal(idx, ri)
    inf = t.info()
    off = _off(M)
    assert inf["nodes"] == nodes.shape[0] and inf["prim_refs"] == idx.shape[0] and inf["M"] == M
    assert inf["leaves"] == int(((nodes[:, 1] & ((1 << off) - 1)) == M).sum())


def test_killeroo_trees_equal_the_restatement(hprt):
    """killeroo-simple (triangles and spheres) at M = 3, the whole scene; and at M = 7 and 13 a deterministic prefix of its
    triangles (the restatement builds single-threaded)"""
    ref = rbsp_ref.RbspScene(KILLEROO, 3)
    t = hprt.Rbsp(hprt.Model.load(KILLEROO), n_directions=3)
    nodes, idx = t.arrays()
    rn, ri = ref.tree()
    assert np.array_equal(nodes, rn) and np.array_equal(idx, ri)
    assert t.info()["nodes"] > 100000 and t.info()["depth"] <= round(2 + 1.6 * 16)
    p9 = ref.triangles()
    assert p9.shape[0] > 50000
    for M in (7, 13):
        _same_tree(hprt, p9[:3000], M)


def _soup(rng, n, grid=None, degenerate=0.0):
    c = rng.uniform(-10, 10, (n, 1, 3))
    e = rng.normal(0, 1.5, (n, 3, 3))
    p = (c + e).astype(np.float32)
    if grid:
        p = (np.round(p / grid) * grid).astype(np.float32)       # equal edge t values, coincident k-DOP edges, in-plane triangles
    k = rng.uniform(size=n) < degenerate
    p[k, 2] = p[k, 0]                                              # zero-area triangles
    p[k[: n // 2].nonzero()[0], 1] = p[k[: n // 2].nonzero()[0], 0]   # and points
    return p.reshape(n, 9)


@pytest.mark.parametrize("M", [3, 7, 9, 13])
@pytest.mark.parametrize("seed", range(3))
def test_random_soups_equal_the_restatement(hprt, M, seed):
    rng = np.random.default_rng(seed)
    _same_tree(hprt, _soup(rng, 600), M)
    _same_tree(hprt, _soup(rng, 600, grid=1.0, degenerate=0.2), M)
    _same_tree(hprt, _soup(rng, 300, grid=4.0, degenerate=0.5), M)


@pytest.mark.parametrize("kw", [dict(max_prims=4), dict(max_depth=5), dict(isect_cost=20, trav_cost=1), dict(empty_bonus=0.5),
                                dict(empty_bonus=1.0, max_depth=30), dict(trav_cost=400)])
def test_non_default_parameters_equal_the_restatement(hprt, kw):
    rng = np.random.default_rng(7)
    for M in (3, 9):
        _same_tree(hprt, _soup(rng, 500, grid=0.5, degenerate=0.1), M, **kw)


def test_tree_is_independent_of_the_thread_count(hprt):
    rng = np.random.default_rng(3)
    p9 = _soup(rng, 4000, grid=0.25, degenerate=0.05)
    for M in (3, 13):
        a = hprt.Rbsp.from_triangles(p9, M, threads=1).arrays()
        b = hprt.Rbsp.from_triangles(p9, M, threads=4).arrays()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), M


def test_two_triangle_tree_by_hand(hprt):
    """A spans x [0, 1], B = A + (3, 0, 0); both span y, z [0, 1].  Only x has edges strictly inside the root: 1 (A's end) and
    3 (B's start).  The k-DOP halves are boxes: areas 6 / 14 at x = 1, 14 / 6 at x = 3, so both cost 5 + 80 (6 + 14) / 22 and
    the first (x = 1) wins: interior {split 1.0, axis 0 | above 2 << 2}, below leaf A, above leaf B."""
    a = np.array([[0, 0, 0], [1, 1, 0], [0, 0, 1]], np.float32)
    p9 = np.stack([a, a + np.float32([3, 0, 0])]).reshape(2, 9)
    nodes, idx = hprt.Rbsp.from_triangles(p9, 3).arrays()
    assert nodes.tolist() == [[_f2u(1.0), 0 | (2 << 2)], [0, 3 | (1 << 2)], [1, 3 | (1 << 2)]]
    assert idx.shape[0] == 0
    rn, _, _ = rbsp_ref.build(p9, 3)
    assert np.array_equal(nodes, rn)


@pytest.mark.parametrize("M", [3, 7, 9, 13])
def test_structural_invariants(hprt, M):
    rng = np.random.default_rng(M)
    p9 = _soup(rng, 1500, grid=0.5, degenerate=0.1)
    t = hprt.Rbsp.from_triangles(p9, M, max_prims=2)
    nodes, idx = t.arrays()
    off = _off(M); mask = (1 << off) - 1
    leaf = (nodes[:, 1] & mask) == M
    assert not leaf[0] and leaf[-1]
    n = nodes.shape[0]
    for k in np.nonzero(~leaf)[0]:
        assert (nodes[k, 1] & mask) < M
        above = nodes[k, 1] >> off
        assert k + 1 < above < n
    for k in np.nonzero(leaf)[0]:
        np_ = nodes[k, 1] >> off
        if np_ == 1:
            assert nodes[k, 0] < p9.shape[0]
        elif np_ > 1:
            assert nodes[k, 0] + np_ <= idx.shape[0]
    assert (idx < p9.shape[0]).all()
    # every primitive is referenced by some leaf
    refs = set(idx.tolist()) | set(nodes[leaf & ((nodes[:, 1] >> off) == 1), 0].tolist())
    assert refs == set(range(p9.shape[0]))
    assert t.info()["depth"] <= round(2 + 1.6 * int(np.log2(p9.shape[0])))


def test_front_end_parameters_and_warnings(hprt, tmp_path):
    from test_host_side import _mesh_scene
    from test_kdtree_fallbacks import INSTANCED_KD
    P = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 1], [3, 0, 1], [2, 1, 1], [0, 2, 2], [1, 3, 2], [0, 3, 3]], np.float32)
    tri = np.arange(9, dtype=np.int32).reshape(3, 3)

    def parse(acc, text=None):
        p = tmp_path / "s.pbrt"
        p.write_text((text or _mesh_scene(P, tri)).replace('Accelerator "bvh"', acc).replace('Accelerator "kdtree"', acc))
        return hprt.Model.parse(str(p))

    m = parse('Accelerator "rbsp"')
    assert m.accelerator == "rbsp"
    assert any("hprt_scene_attach_rbsp" in w for w in m.warnings())
    assert not any("outside the hot-path scope" in w for w in m.warnings())
    p9 = P[tri].reshape(-1, 9)
    # defaults 80 / 5 / 0 / 1 / -1, nbDirections 3
    assert np.array_equal(hprt.Rbsp(m).arrays()[0], hprt.Rbsp.from_triangles(p9).arrays()[0])
    m2 = parse('Accelerator "rbsp" "integer nbDirections" [7] "float splitalpha" [10] "integer alphatype" [1] "integer axisselectiontype" [2] '
               '"integer axisselectionamount" [3] "integer maxprims" [2] "integer maxdepth" [3] "integer intersectcost" [20] '
               '"integer traversalcost" [2] "float emptybonus" [0.5]')
    assert not any("not used" in w for w in m2.warnings()), m2.warnings()
    t2 = hprt.Rbsp(m2)
    assert t2.info()["M"] == 7
    assert np.array_equal(t2.arrays()[0], hprt.Rbsp.from_triangles(p9, 7, 20, 2, 0.5, 2, 3).arrays()[0])
    # explicit parameters override the scene's line
    assert hprt.Rbsp(m2, n_directions=3).info()["M"] == 3
    # an unsupported direction count is refused, from the scene and from the parameters
    with pytest.raises(hprt.HprtError) as e:
        hprt.Rbsp(parse('Accelerator "rbsp" "integer nbDirections" [5]'))
    assert e.value.code == hprt.E_UNSUPPORTED
    for M in (0, 1, 5, 100, 107, -1):
        with pytest.raises(hprt.HprtError) as e:
            hprt.Rbsp.from_triangles(p9, M)
        assert e.value.code == hprt.E_UNSUPPORTED, M
    # instanced rbsp scenes keep the BVH and today's warning; the build is refused
    mi = parse('Accelerator "rbsp"', INSTANCED_KD)
    assert mi.accelerator == "rbsp"
    assert any('"rbsp" is outside the hot-path scope; "bvh" used' in w for w in mi.warnings())
    with pytest.raises(hprt.HprtError) as e:
        hprt.Rbsp(mi)
    assert e.value.code == hprt.E_UNSUPPORTED
    # nothing changes for "bvh" and "kdtree" scenes
    assert not any("rbsp" in w for w in parse('Accelerator "kdtree"').warnings())
    assert parse('Accelerator "bvh" "integer nbDirections" [7]').warnings() == parse('Accelerator "bvh"').warnings()


CHECK_DRIVER = r"""
#include <cstdio>
#include <cstring>
#include "rbsp_builder.h"
using namespace hprt;
static int fails = 0;
static void expect(const RbspTree &t, const char *want, uint32_t depth = 0) {
    uint32_t d = 12345;
    const char *got = CheckRbspTree(t, &d);
    if (std::strstr(got, want) == nullptr || (!*want && d != depth)) { std::printf("want '%s' got '%s' depth %u\n", want, got, d); ++fails; }
}
static const uint32_t M = 7, OFF = 3;
static RbspNode leaf(uint32_t np, uint32_t a) { return RbspNode{a, M | (np << OFF)}; }
static RbspNode interior(uint32_t axis, uint32_t above) { return RbspNode{0x3f800000u, axis | (above << OFF)}; }
int main() {
    RbspTree t; t.nPrims = 3; t.M = M; RbspDirections(M, &t.directions);
    t.nodes = {interior(5, 2), leaf(1, 0), leaf(2, 0)}; t.primIndices = {1, 2};
    expect(t, "", 1);
    RbspTree e = t; e.nodes.clear(); expect(e, "no nodes");
    e = t; e.nodes = {interior(0, 2)}; expect(e, "no below child");
    e = t; e.nodes[0] = interior(1, 1); expect(e, "above child is out of range");
    e = t; e.nodes[0] = interior(1, 3); expect(e, "above child is out of range");
    e = t; e.nodes[1] = leaf(1, 3); expect(e, "one-primitive leaf");
    e = t; e.nodes[2] = leaf(2, 1); expect(e, "runs past primitiveIndices");
    e = t; e.primIndices = {1, 7}; expect(e, "primitiveIndices names");
    e = t; e.M = 5; expect(e, "not 3, 7, 9 or 13");
    e = t; e.directions.pop_back(); expect(e, "direction table");
    // a chain of 70 interior levels: the depth the attach step compares with the todo capacity (64)
    e = t; e.nodes.clear(); e.primIndices.clear();
    for (uint32_t k = 0; k < 70; ++k) { e.nodes.push_back(interior(k % M, 2 * k + 2)); e.nodes.push_back(leaf(0, 0)); }
    e.nodes.push_back(leaf(0, 0));
    expect(e, "", 70);
    return fails;
}
"""


def test_attach_check_rejects_malformed_trees(tmp_path):
    """CheckRbspTree (csrc/rbsp_builder.cpp) is what hprt_scene_attach_rbsp applies before anything reaches the device (and
    the depth it returns is held to HPRT_RBSP_MAX_DEPTH); the builders cannot produce a malformed tree, so it is driven here
    directly, built from the library's own source."""
    src = tmp_path / "check.cpp"
    src.write_text(CHECK_DRIVER)
    csrc = os.path.join(ROOT, "thesis-pbrt-v3_amd", "csrc")
    exe = str(tmp_path / "check")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-pthread", "-I" + csrc, str(src), os.path.join(csrc, "rbsp_builder.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout


def test_pixel_stats_files_of_an_rbsp_render(hprt, tmp_path):
    st = np.arange(3 * 4 * 7, dtype=np.uint64).reshape(3, 4, 7)
    hprt.write_pixel_stats_accel(str(tmp_path / "rb"), st, hprt.ACCEL_RBSP)
    names = sorted(p.name for p in tmp_path.iterdir())
    assert names == sorted("rb-%s.txt" % n for n in ("primitiveIntersections", "primitiveIntersectionsP", "kdTreeNodeTraversals", "kdTreeNodeTraversalsP",
                                                   "bspTreeNodeTraversals", "bspTreeNodeTraversalsP", "leafNodeTraversals", "leafNodeTraversalsP"))
    assert np.array_equal(np.loadtxt(tmp_path / "rb-bspTreeNodeTraversals.txt", dtype=np.uint64), st[:, :, 5])
    assert np.array_equal(np.loadtxt(tmp_path / "rb-bspTreeNodeTraversalsP.txt", dtype=np.uint64), st[:, :, 6])
    assert np.array_equal(np.loadtxt(tmp_path / "rb-leafNodeTraversals.txt", dtype=np.uint64), st[:, :, 3])
    assert np.loadtxt(tmp_path / "rb-kdTreeNodeTraversals.txt").sum() == 0
    assert np.loadtxt(tmp_path / "rb-kdTreeNodeTraversalsP.txt").sum() == 0
