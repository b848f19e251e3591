"""Accelerator "rbspkd" on the host: the kd-aware builder (RBSPKd::buildTree) against the test-side restatement
(tests/rbspkd_reference.cpp) node for node, thread-count independence, trees that mix kd and oblique interior nodes, the
difference from the RBSP tree, the front end's parameters and warnings, the refusals, the structural check behind attach and the
fork's four traversal matrices for an rbspkd render.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, KILLEROO, ROOT
from tree_ref import rbspkd as rbspkd_ref

DODECA = os.path.join(GOLDEN, "dodecahedron.hprt")


def _kinds(nodes, M):
    """(kd interior nodes, oblique interior nodes) of a node array"""
    ax = nodes[:, 1] & ((1 << M.bit_length()) - 1)
    return int((ax < 3).sum()), int(((ax >= 3) & (ax != M)).sum())


def _same_tree(hprt, p9, M, **kw):
    t = hprt.RbspKd.from_triangles(p9, M, **kw)
    nodes, idx = t.arrays()
    rn, ri, rd = rbspkd_ref.build(p9, M, **kw)
    assert nodes.shape == rn.shape and np.array_equal(nodes, rn), (nodes.shape, rn.shape)
    assert np.array_equal(idx, ri)
    assert np.array_equal(t.directions().view(np.uint32), rd.view(np.uint32))
    inf = t.info()
    assert (inf["kd_interior"], inf["bsp_interior"]) == _kinds(nodes, M)
    return t, nodes, idx


@pytest.mark.parametrize("M", [3, 7, 9, 13])
def test_dodecahedron_trees_equal_the_restatement(hprt, M):
    m = hprt.Model.load(DODECA)
    t = hprt.RbspKd(m, n_directions=M)
    nodes, idx = t.arrays()
    rn, ri = rbspkd_ref.RbspKdScene(DODECA, M).tree()
    assert np.array_equal(nodes, rn) and np.array_equal(idx, ri)
    inf = t.info()
    assert inf["nodes"] == nodes.shape[0] and inf["prim_refs"] == idx.shape[0] and inf["M"] == M
    kd, bsp = _kinds(nodes, M)
    assert (inf["kd_interior"], inf["bsp_interior"]) == (kd, bsp)
    assert inf["leaves"] + kd + bsp == inf["nodes"]
    if M == 3:
        assert bsp == 0 and kd > 0
    else:
        assert kd > 0 and bsp > 0, (kd, bsp)       # both kinds: the test cannot pass on a tree of one kind only


@pytest.mark.parametrize("M", [3, 7, 9, 13])
def test_rbspkd_tree_differs_from_the_rbsp_tree(hprt, M):
    m = hprt.Model.load(DODECA)
    a = hprt.RbspKd(m, n_directions=M).arrays()[0]
    b = hprt.Rbsp(m, n_directions=M).arrays()[0]
    assert a.shape != b.shape or not np.array_equal(a, b)
    # M = 3: the RBSP-3 tree costed with kdtraversalcost — so with kdtraversalcost = traversalcost the two are the same tree
    if M == 3:
        p9 = rbspkd_ref.RbspKdScene(DODECA, 3, build=False).triangles()
        assert np.array_equal(hprt.RbspKd.from_triangles(p9, 3, kd_trav_cost=5).arrays()[0], hprt.Rbsp.from_triangles(p9, 3).arrays()[0])


def test_killeroo_trees_equal_the_restatement(hprt):
    """killeroo-simple (triangles and spheres) at M = 3, the whole scene; at M = 7 and 13 a deterministic prefix of its
    triangles (the restatement builds single-threaded)"""
    ref = rbspkd_ref.RbspKdScene(KILLEROO, 3)
    t = hprt.RbspKd(hprt.Model.load(KILLEROO), n_directions=3)
    nodes, idx = t.arrays()
    rn, ri = ref.tree()
    assert np.array_equal(nodes, rn) and np.array_equal(idx, ri)
    assert t.info()["nodes"] > 100000
    p9 = ref.triangles()
    for M in (7, 13):
        _, nodes, _ = _same_tree(hprt, p9[:3000], M)
        kd, bsp = _kinds(nodes, M)
        assert kd > 0 and bsp > 0, (M, kd, bsp)


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


@pytest.mark.parametrize("kw", [dict(kd_trav_cost=1), dict(kd_trav_cost=5), dict(kd_trav_cost=20), dict(max_prims=4), dict(max_depth=5),
                                dict(isect_cost=20, trav_cost=1), dict(empty_bonus=0.5), dict(empty_bonus=1.0, max_depth=30),
                                dict(trav_cost=400, kd_trav_cost=3)])
def test_non_default_parameters_equal_the_restatement(hprt, kw):
    rng = np.random.default_rng(7)
    for M in (3, 9, 13):
        _same_tree(hprt, _soup(rng, 500, grid=0.5, degenerate=0.1), M, **kw)


def test_tree_is_independent_of_the_thread_count(hprt):
    rng = np.random.default_rng(3)
    p9 = _soup(rng, 4000, grid=0.25, degenerate=0.05)
    for M in (3, 13):
        a = hprt.RbspKd.from_triangles(p9, M, threads=1).arrays()
        b = hprt.RbspKd.from_triangles(p9, M, threads=4).arrays()
        c = hprt.RbspKd.from_triangles(p9, M, threads=16).arrays()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[0], c[0]), M


def test_front_end_parameters_and_warnings(hprt, tmp_path):
    from test_host_side import _mesh_scene
    from test_kdtree_fallbacks import INSTANCED_KD
    P = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 1], [3, 0, 1], [2, 1, 1], [0, 2, 2], [1, 3, 2], [0, 3, 3]], np.float32)
    tri = np.arange(9, dtype=np.int32).reshape(3, 3)

    def parse(acc, text=None):
        p = tmp_path / "s.pbrt"
        p.write_text((text or _mesh_scene(P, tri)).replace('Accelerator "bvh"', acc).replace('Accelerator "kdtree"', acc))
        return hprt.Model.parse(str(p))

    m = parse('Accelerator "rbspkd"')
    assert m.accelerator == "rbspkd"
    assert any("hprt_scene_attach_rbspkd" in w for w in m.warnings())
    assert not any("outside the hot-path scope" in w for w in m.warnings())
    p9 = P[tri].reshape(-1, 9)
    # defaults 80 / 5 / kd 1 / 0 / 1 / -1, nbDirections 3
    assert np.array_equal(hprt.RbspKd(m).arrays()[0], hprt.RbspKd.from_triangles(p9).arrays()[0])
    m2 = parse('Accelerator "rbspkd" "integer nbDirections" [7] "float splitalpha" [10] "integer alphatype" [1] "integer axisselectiontype" [2] '
               '"integer axisselectionamount" [3] "integer maxprims" [2] "integer maxdepth" [3] "integer intersectcost" [20] '
               '"integer traversalcost" [2] "integer kdtraversalcost" [4] "float emptybonus" [0.5]')
    assert not any("not used" in w for w in m2.warnings()), m2.warnings()
    t2 = hprt.RbspKd(m2)
    assert t2.info()["M"] == 7
    assert np.array_equal(t2.arrays()[0], hprt.RbspKd.from_triangles(p9, 7, 20, 2, 4, 0.5, 2, 3).arrays()[0])
    assert hprt.RbspKd(m2, n_directions=3).info()["M"] == 3
    # "kdtraversalcost" is read by rbspkd only: an rbsp scene reports it unused, as the reference's ParamSet would
    assert any("kdtraversalcost" in w for w in parse('Accelerator "rbsp" "integer kdtraversalcost" [4]').warnings())
    with pytest.raises(hprt.HprtError) as e:
        hprt.RbspKd(parse('Accelerator "rbspkd" "integer nbDirections" [5]'))
    assert e.value.code == hprt.E_UNSUPPORTED
    for M in (0, 1, 5, 100, -1):
        with pytest.raises(hprt.HprtError) as e:
            hprt.RbspKd.from_triangles(p9, M)
        assert e.value.code == hprt.E_UNSUPPORTED, M
    # instanced rbspkd scenes keep the BVH and the out-of-scope warning; the build is refused
    mi = parse('Accelerator "rbspkd"', INSTANCED_KD)
    assert mi.accelerator == "rbspkd"
    assert any('"rbspkd" is outside the hot-path scope; "bvh" used' in w for w in mi.warnings())
    with pytest.raises(hprt.HprtError) as e:
        hprt.RbspKd(mi)
    assert e.value.code == hprt.E_UNSUPPORTED
    # nothing changes for "bvh", "kdtree" and "rbsp" scenes
    assert not any("rbspkd" in w for w in parse('Accelerator "rbsp"').warnings())
    assert any("kdtraversalcost" in w and "not used" in w for w in parse('Accelerator "bvh" "integer kdtraversalcost" [7]').warnings())


CHECK_DRIVER = r"""
#include <cstdio>
#include <cstring>
#include <random>
#include "rbsp_builder.h"
using namespace hprt;
static int fails = 0;
static void expect(const RbspTree &t, const char *want) {
    uint32_t d = 0;
    const char *got = CheckRbspTree(t, &d);
    if (std::strstr(got, want) == nullptr) { std::printf("want '%s' got '%s'\n", want, got); ++fails; }
}
int main() {
    // a kd-aware tree from the builder over a random soup at M = 13, then the same tree broken in each way attach refuses
    std::mt19937 rng(5);
    std::uniform_real_distribution<float> u(-5.f, 5.f);
    const size_t n = 300;
    std::vector<float> p9(9 * n), lo(3 * n), hi(3 * n);
    for (auto &v : p9) v = u(rng);
    for (size_t i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a) {
            const float x = p9[9 * i + a], y = p9[9 * i + 3 + a], z = p9[9 * i + 6 + a];
            lo[3 * i + a] = std::min(std::min(x, y), z); hi[3 * i + a] = std::max(std::max(x, y), z);
        }
    std::vector<uint8_t> isTri(n, 1);
    RbspParams p; p.kdAware = true; p.nDirections = 13; p.threads = 2;
    RbspTree t;
    if (!BuildRbspTree(n, lo.data(), hi.data(), p9.data(), isTri.data(), p, &t).empty()) { std::printf("build failed\n"); return 1; }
    uint32_t kd = 0, bsp = 0;
    RbspInteriorCounts(t, &kd, &bsp);
    if (kd == 0 || bsp == 0) { std::printf("kd %u bsp %u\n", kd, bsp); ++fails; }
    expect(t, "");
    const uint32_t off = RbspBitOffset(13), mask = RbspBitMask(13);
    size_t inner = 0, one = 0, multi = 0;
    for (size_t k = 0; k < t.nodes.size(); ++k) {
        const uint32_t ax = t.nodes[k].b & mask, np = t.nodes[k].b >> off;
        if (ax != 13 && !inner) inner = k + 1;
        if (ax == 13 && np == 1 && !one) one = k + 1;
        if (ax == 13 && np > 1 && !multi) multi = k + 1;
    }
    if (!inner || !one || !multi) { std::printf("tree lacks a node kind\n"); return 1; }
    RbspTree e = t; e.nodes[inner - 1].b = (e.nodes[inner - 1].b & mask) | ((uint32_t)(inner - 1) << off); expect(e, "above child is out of range");
    e = t; e.nodes[inner - 1].b = (e.nodes[inner - 1].b & mask) | ((uint32_t)t.nodes.size() << off); expect(e, "above child is out of range");
    e = t; e.nodes[inner - 1].b = (e.nodes[inner - 1].b & ~mask) | 14u; expect(e, "direction is out of range");
    e = t; e.nodes[one - 1].a = (uint32_t)n; expect(e, "one-primitive leaf");
    e = t; e.nodes[multi - 1].a = (uint32_t)t.primIndices.size(); expect(e, "runs past primitiveIndices");
    e = t; e.primIndices[0] = (uint32_t)n + 3; expect(e, "primitiveIndices names");
    e = t; e.M = 11; expect(e, "not 3, 7, 9 or 13");
    e = t; e.directions.resize(21); expect(e, "direction table");
    e = t; e.nodes.resize(1); e.nodes[0] = t.nodes[inner - 1]; expect(e, "no below child");
    return fails;
}
"""


def test_attach_check_rejects_malformed_trees(tmp_path):
    """hprt_scene_attach_rbspkd applies CheckRbspTree before anything reaches the device; it is driven here on a kd-aware tree
    from the library's own builder, broken in each way the check refuses."""
    src = tmp_path / "check.cpp"
    src.write_text(CHECK_DRIVER)
    csrc = os.path.join(ROOT, "thesis-pbrt-v3_amd", "csrc")
    exe = str(tmp_path / "check")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-pthread", "-I" + csrc, str(src), os.path.join(csrc, "rbsp_builder.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout


def test_four_traversal_matrices_of_an_rbspkd_render(hprt, tmp_path):
    """Film::WriteGeneralStats for an rbspkd render (core/film.cpp:174-177): kd from the kd planes, bsp = slot - kd."""
    rng = np.random.default_rng(1)
    st = rng.integers(0, 1000, (3, 4, 7)).astype(np.uint64)
    kd2 = np.stack([st[:, :, 5] // 3, st[:, :, 6] // 2]).astype(np.uint64)
    hprt.write_pixel_stats_rbspkd(str(tmp_path / "rk"), st, kd2)
    names = sorted(p.name for p in tmp_path.iterdir())
    assert names == sorted("rk-%s.txt" % n for n in ("primitiveIntersections", "primitiveIntersectionsP", "kdTreeNodeTraversals", "kdTreeNodeTraversalsP",
                                                   "bspTreeNodeTraversals", "bspTreeNodeTraversalsP", "leafNodeTraversals", "leafNodeTraversalsP"))
    load = lambda n: np.loadtxt(tmp_path / ("rk-%s.txt" % n), dtype=np.uint64).reshape(3, 4)
    assert np.array_equal(load("kdTreeNodeTraversals"), kd2[0]) and np.array_equal(load("kdTreeNodeTraversalsP"), kd2[1])
    assert np.array_equal(load("bspTreeNodeTraversals"), st[:, :, 5] - kd2[0])
    assert np.array_equal(load("bspTreeNodeTraversalsP"), st[:, :, 6] - kd2[1])
    assert np.array_equal(load("primitiveIntersections"), st[:, :, 1]) and np.array_equal(load("leafNodeTraversalsP"), st[:, :, 4])
    bad = kd2.copy(); bad[0, 0, 0] = st[0, 0, 5] + 1
    with pytest.raises(hprt.HprtError) as e:
        hprt.write_pixel_stats_rbspkd(str(tmp_path / "bad"), st, bad)
    assert e.value.code == hprt.E_INVALID
