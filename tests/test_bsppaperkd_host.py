"""Accelerator "bsppaperkd" on the host: the builder against the test-side restatement (tests/bsppaperkd_reference.cpp) node for
node (flags, split, the axis of plane nodes) and in primitiveIndices — the dodecahedron, random and grid-snapped soups, a prefix of
killeroo-simple, two small scenes whose choices are known, non-default parameters — with both node kinds asserted present where
both are claimed covered; thread-count independence; the front end's parameters and warnings; bsppaper trees unchanged; the
refusals and the structural check behind attach.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, KILLEROO, ROOT
from tree_ref import bsppaper as bsppaper_ref
import bsppaperkd_ref as kdref
from test_bsppaper_host import _soup

DODECA = os.path.join(GOLDEN, "dodecahedron.hprt")


def _same_tree(hprt, p9, both_kinds=True, **kw):
    t = hprt.BspPaperKd.from_triangles(p9, **kw)
    nodes, idx = t.arrays()
    kdref.assert_same_tree((nodes, idx), kdref.build(p9, **kw))
    kind, kd, plane, leaves = kdref.kinds(nodes)
    assert not nodes[kind != kdref.PLANE, 2:].any()             # kd nodes and leaves: the axis words are written as zero
    inf = t.info()
    assert (inf["nodes"], inf["prim_refs"], inf["leaves"], inf["kd_interior"], inf["plane_interior"]) == (nodes.shape[0], idx.shape[0], leaves, kd, plane)
    if both_kinds:
        assert kd > 0 and plane > 0, (kd, plane)                  # else the comparison would not cover both interior forms
    return t, nodes, idx


def test_dodecahedron_tree_equals_the_restatement(hprt):
    t = hprt.BspPaperKd(hprt.Model.load(DODECA))
    nodes, idx = t.arrays()
    kdref.assert_same_tree((nodes, idx), kdref.BspKdScene(DODECA).tree())
    _, kd, plane, leaves = kdref.kinds(nodes)
    assert kd > 0 and plane > 0
    assert t.info() == dict(nodes=nodes.shape[0], leaves=leaves, depth=t.info()["depth"], prim_refs=idx.shape[0], kd_interior=kd, plane_interior=plane)


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


@pytest.mark.parametrize("kw", [dict(kd_trav_cost=1), dict(kd_trav_cost=5), dict(kd_trav_cost=20), dict(trav_cost=1), dict(trav_cost=40, kd_trav_cost=5),
                                dict(max_prims=2), dict(max_depth=4), dict(empty_bonus=0.5), dict(isect_cost=20, trav_cost=2, kd_trav_cost=2)])
def test_non_default_parameters_equal_the_restatement(hprt, kw):
    # (four levels over 200 triangles never reach a node small enough for a plane to pay its penalty: kd nodes only there)
    _same_tree(hprt, _soup(np.random.default_rng(7), 200, grid=0.25), both_kinds="max_depth" not in kw, **kw)


def test_kdtraversalcost_changes_the_tree(hprt):
    p9 = _soup(np.random.default_rng(7), 200, grid=0.25)
    a = hprt.BspPaperKd.from_triangles(p9, kd_trav_cost=1).arrays()[0]
    b = hprt.BspPaperKd.from_triangles(p9, kd_trav_cost=20).arrays()[0]
    assert a.shape != b.shape or not np.array_equal(a, b)


def test_tree_is_independent_of_the_thread_count(hprt):
    p9 = _soup(np.random.default_rng(11), 1500)
    a = hprt.BspPaperKd.from_triangles(p9, threads=1).arrays()
    b = hprt.BspPaperKd.from_triangles(p9, threads=16).arrays()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    _, kd, plane, _ = kdref.kinds(a[0])
    assert kd > 0 and plane > 0


# tests/test_bsppaper_host.py's two triangles in z = 0 on either side of the diagonal x = y, a quarter off it
A = np.array([[0.25, 0, 0], [1, 0, 0], [1, 0.75, 0]], np.float32)
B = np.array([[0, 0.25, 0], [0.75, 1, 0], [0, 1, 0]], np.float32)


def test_a_triangle_plane_wins_despite_the_penalty(hprt):
    """At the root (N = 2) a plane candidate pays BSP_ALPHA * isectCost * (N - 1) + kdTraversalCost = 0.1 * 80 + 1 = 9 where
    bsppaper paid traversalCost = 5, an axis candidate 1.  Every axis plane leaves a triangle on both sides; B's edge plane,
    axis (1, -1, 0) / sqrt 2 at t = -0.25 / sqrt 2, cuts B off, and still wins: the root is the plane node bsppaper's root is,
    with B alone below it."""
    p9 = np.stack([A, B]).reshape(2, 9)
    t, nodes, idx = _same_tree(hprt, p9)
    paper = hprt.BspPaper.from_triangles(p9).arrays()[0]
    assert nodes[0, 1] & 7 == kdref.PLANE and nodes[0, 1] >> 3 == 2
    assert np.array_equal(nodes[0, [0, 2, 3, 4]], paper[0, [0, 2, 3, 4]])            # the same split and axis
    s = nodes[0, 2:].view(np.float32)
    assert s[0] > 0.7 and s[1] == -s[0] and s[2] == 0 and nodes[0, :1].view(np.float32)[0] == np.float32(-0.25) * s[0]
    assert nodes[1, 1] == (kdref.LEAF | 1 << 3) and nodes[1, 0] == 1                 # leaf: B


def test_the_penalty_flips_a_plane_choice_to_an_axis(hprt):
    """The root's above child holds A and B again.  bsppaper takes A's edge plane there (t = +0.25 / sqrt 2); with the penalty
    of 9 against an axis split's 1 the kd-aware tree takes the axis plane y = 0.75 instead — a kd node — and A's edge plane only
    one level further down."""
    p9 = np.stack([A, B]).reshape(2, 9)
    _, nodes, _ = _same_tree(hprt, p9)
    paper = hprt.BspPaper.from_triangles(p9).arrays()[0]
    assert paper[2, 1] & 1 == 0 and paper[2, 2:].view(np.float32)[1] < 0             # bsppaper: the oblique plane
    assert nodes[2, 1] & 7 == 1 and nodes[2, :1].view(np.float32)[0] == np.float32(0.75)      # bsppaperkd: kd node, axis y
    assert not nodes[2, 2:].any()
    assert nodes[3, 1] & 7 == kdref.PLANE and np.array_equal(nodes[3, [0, 2, 3, 4]], paper[2, [0, 2, 3, 4]])


def test_bsppaper_trees_are_unchanged(hprt):
    for seed in range(2):
        p9 = _soup(np.random.default_rng(300 + seed), 200, grid=0.5 if seed else None)
        nodes, idx = hprt.BspPaper.from_triangles(p9).arrays()
        rn, ri = bsppaper_ref.build(p9)
        interior = (nodes[:, 1] & 1) == 0
        assert np.array_equal(nodes[:, :2], rn[:, :2]) and np.array_equal(nodes[interior], rn[interior]) and np.array_equal(idx, ri)


def test_front_end_parameters_and_warnings(hprt, tmp_path):
    from test_host_side import _mesh_scene
    from test_kdtree_fallbacks import INSTANCED_KD
    P = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 1], [3, 0, 1], [2, 1, 1], [0, 2, 2], [1, 3, 2], [0, 3, 3]], np.float32)
    tri = np.arange(9, dtype=np.int32).reshape(3, 3)

    def parse(acc, text=None):
        p = tmp_path / "s.pbrt"
        p.write_text((text or _mesh_scene(P, tri)).replace('Accelerator "bvh"', acc).replace('Accelerator "kdtree"', acc))
        return hprt.Model.parse(str(p))

    m = parse('Accelerator "bsppaperkd"')
    assert m.accelerator == "bsppaperkd"
    assert any("hprt_bsppaperkd_build" in w and "hprt_scene_attach_bsppaperkd" in w for w in m.warnings()), m.warnings()
    assert not any("outside the hot-path scope" in w for w in m.warnings())
    p9 = P[tri].reshape(-1, 9)
    assert np.array_equal(hprt.BspPaperKd(m).arrays()[0], hprt.BspPaperKd.from_triangles(p9).arrays()[0])
    m2 = parse('Accelerator "bsppaperkd" "integer nbDirections" [7] "integer maxprims" [2] "integer maxdepth" [3] "integer intersectcost" [20] '
               '"integer traversalcost" [2] "integer kdtraversalcost" [4] "float emptybonus" [0.5]')
    assert not any("not used" in w for w in m2.warnings()), m2.warnings()
    assert np.array_equal(hprt.BspPaperKd(m2).arrays()[0], hprt.BspPaperKd.from_triangles(p9, 20, 2, 4, 0.5, 2, 3).arrays()[0])
    m3 = parse('Accelerator "bsppaperkd" "integer bogus" [1]')
    assert any('"integer bogus" of Accelerator not used' in w for w in m3.warnings()), m3.warnings()
    # "kdtraversalcost" belongs to the kd-aware trees only
    m4 = parse('Accelerator "bsppaper" "integer kdtraversalcost" [4]')
    assert any('"integer kdtraversalcost" of Accelerator not used' in w for w in m4.warnings()), m4.warnings()
    # explicit parameters override the scene's line
    assert np.array_equal(hprt.BspPaperKd(m2, isect_cost=80).arrays()[0], hprt.BspPaperKd.from_triangles(p9).arrays()[0])
    # instanced scenes keep the BVH and the warning; the build is refused
    mi = parse('Accelerator "bsppaperkd"', INSTANCED_KD)
    assert any('"bsppaperkd" is outside the hot-path scope; "bvh" used' in w for w in mi.warnings())
    assert not any("hprt_scene_attach_bsppaperkd" in w for w in mi.warnings())
    with pytest.raises(hprt.HprtError) as e:
        hprt.BspPaperKd(mi)
    assert e.value.code == hprt.E_UNSUPPORTED


def test_primitive_buffer_limit_stays_checked(hprt):
    """The (maxDepth + 1) * N slots suffice for every input, so the check is a guard that a build never trips: a node at level d
    (the root is 0) starts at most d * N slots in (each ancestor put at most its own above share, at most N, before it), it is
    split only at d <= maxDepth - 1, and its two shares take at most 2 * N slots.  Triangles that all span the whole box straddle
    every split, which is the worst case; shallow and deep limits both build, and equal the restatement, which writes the
    reference's buffer."""
    rng = np.random.default_rng(5)
    p9 = rng.uniform(-1, 1, (40, 3, 3)).astype(np.float32)
    p9[:, 0] = -1 + 0.01 * rng.uniform(0, 1, (40, 3)); p9[:, 1] = 1 - 0.01 * rng.uniform(0, 1, (40, 3))     # corner to corner
    p9 = p9.reshape(40, 9)
    for max_depth in (1, 2, 3, 63):
        t, nodes, idx = _same_tree(hprt, p9, both_kinds=False, max_depth=max_depth, empty_bonus=0.9)
        assert t.info()["depth"] <= max_depth and idx.shape[0] <= (max_depth + 1) * 40


CHECK_DRIVER = r"""
#include <cstdio>
#include <cstring>
#include "bsppaper_builder.h"
using namespace hprt;
static int fails = 0;
static void expect(const BspPaperTree &t, const char *want, uint32_t depth = 0) {
    uint32_t d = 12345;
    const char *got = CheckBspPaperKdTree(t, &d);
    if (std::strstr(got, want) == nullptr || (!*want && d != depth)) { std::printf("want '%s' got '%s' depth %u\n", want, got, d); ++fails; }
}
static BspNode leaf(uint32_t np, uint32_t a) { return BspNode{a, 3u | (np << 3)}; }
static BspNode kd(uint32_t axis, uint32_t above) { return BspNode{0x3f800000u, axis | (above << 3)}; }
static BspNode plane(uint32_t above) { return BspNode{0x3f800000u, 4u | (above << 3)}; }
int main() {
    BspPaperTree t; t.nPrims = 3; t.kdAware = true;
    // plane root, kd node below it, three leaves
    t.nodes = {plane(4), kd(2, 3), leaf(1, 0), leaf(0, 0), leaf(2, 0)}; t.primIndices = {1, 2};
    t.axes = {0.6f, 0.8f, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    expect(t, "", 2);
    BspPaperTree e = t; e.nodes.clear(); e.axes.clear(); expect(e, "no nodes");
    e = t; e.nodes[0] = plane(1); expect(e, "above child is out of range");
    e = t; e.nodes[1] = kd(0, 5); expect(e, "above child is out of range");
    e = t; e.nodes[1].b = 5u | (3u << 3); expect(e, "node kind");
    e = t; e.nodes[1].b = 7u | (3u << 3); expect(e, "node kind");
    e = t; e.nodes[2] = leaf(1, 3); expect(e, "one-primitive leaf");
    e = t; e.nodes[4] = leaf(2, 1); expect(e, "runs past primitiveIndices");
    e = t; e.primIndices = {1, 7}; expect(e, "primitiveIndices names");
    e = t; e.axes.pop_back(); expect(e, "one axis per node");
    e = t; e.axes[0] = 0; e.axes[1] = 0; expect(e, "axis is zero");
    e = t; e.axes[1] = 1.f / 0.f; expect(e, "not finite");
    e = t; e.axes[3] = 1.f / 0.f; expect(e, "", 2);                      // a kd node's axis words are never read
    // a chain of 70 interior levels, kd and plane nodes alternating: the depth the attach step compares with the todo capacity (64)
    e = t; e.nodes.clear(); e.primIndices.clear(); e.axes.clear();
    for (uint32_t k = 0; k < 70; ++k) { e.nodes.push_back(k % 2 ? plane(2 * k + 2) : kd(k % 3, 2 * k + 2)); e.nodes.push_back(leaf(0, 0)); }
    e.nodes.push_back(leaf(0, 0));
    for (size_t k = 0; k < e.nodes.size(); ++k) { e.axes.push_back(1); e.axes.push_back(0); e.axes.push_back(0); }
    expect(e, "", 70);
    return fails;
}
"""


def test_attach_check_rejects_malformed_trees(hprt, tmp_path):
    """CheckBspPaperKdTree (csrc/bsppaper_builder.cpp) is what hprt_scene_attach_bsppaperkd applies before anything reaches the
    device (and the depth it returns is held to HPRT_BSPPAPERKD_MAX_DEPTH = 64: the depth-70 chain is well-formed and refused
    there as unsupported); driven directly, built from the library's own source."""
    src = tmp_path / "check.cpp"
    src.write_text(CHECK_DRIVER)
    csrc = os.path.join(ROOT, "thesis-pbrt-v3_amd", "csrc")
    exe = str(tmp_path / "check")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-pthread", "-I" + csrc, str(src), os.path.join(csrc, "bsppaper_builder.cpp"),
                        os.path.join(csrc, "bvh_builder.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    header = open(os.path.join(ROOT, "include", "hprt.h")).read()
    assert "#define HPRT_BSPPAPERKD_MAX_DEPTH 64" in header
