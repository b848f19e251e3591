"""Accelerator "kdtree" on the host: the builder against the test-side restatement (tests/kd_reference.cpp) node for node,
a tree worked out by hand, structural invariants, the front end's parameters, the attach step's refusals and the fork's
pixel-statistics files for a kd render.  No GPU needed."""
import os
import struct

import numpy as np
import pytest

from conftest import GOLDEN, KILLEROO
from tree_ref import kd as kd_ref

DODECA = os.path.join(GOLDEN, "dodecahedron.hprt")


def _f2u(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def _same_tree(hprt, lo, hi, **kw):
    t = hprt.KdTree.from_bounds(lo, hi, **kw)
    nodes, idx = t.arrays()
    rn, ri = kd_ref.build(lo, hi, **kw)
    assert nodes.shape == rn.shape and np.array_equal(nodes, rn), (nodes.shape, rn.shape)
    assert np.array_equal(idx, ri)
    return t, nodes, idx


@pytest.mark.parametrize("path", [KILLEROO, DODECA])
def test_scene_trees_equal_the_restatement(hprt, path):
    ref = kd_ref.KdScene(path)
    lo, hi = ref.bounds()
    m = hprt.Model.load(path)
    t = hprt.KdTree(m)                            # the model's parameters: a baked scene has the defaults
    nodes, idx = t.arrays()
    rn, ri = ref.tree()
    assert np.array_equal(nodes, rn) and np.array_equal(idx, ri)
    # the same from the bounds the BVH builder uses
    _same_tree(hprt, lo, hi)
    inf = t.info()
    assert inf["nodes"] == nodes.shape[0] and inf["prim_refs"] == idx.shape[0]
    assert inf["leaves"] == int(((nodes[:, 1] & 3) == 3).sum())
    assert 0 < inf["depth"] <= round(2 + 1.6 * int(np.log2(lo.shape[0])))


def _random_boxes(rng, n, flat=0.0, point=0.0, grid=None):
    c = rng.uniform(-10, 10, (n, 3)).astype(np.float32)
    if grid:
        c = np.round(c / grid) * grid          # many equal edge coordinates
    e = rng.uniform(0, 2, (n, 3)).astype(np.float32)
    if grid:
        e = np.round(e / grid) * grid
    k = rng.uniform(size=n)
    e[k < flat, rng.integers(0, 3)] = 0
    e[k > 1 - point] = 0
    return c.astype(np.float32), (c + e).astype(np.float32)


@pytest.mark.parametrize("seed", range(6))
def test_random_trees_equal_the_restatement(hprt, seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 3000))
    lo, hi = _random_boxes(rng, n, flat=0.2, point=0.1, grid=0.5 if seed % 2 else None)
    _same_tree(hprt, lo, hi)


@pytest.mark.parametrize("kw", [dict(max_prims=4), dict(max_depth=5), dict(max_depth=30), dict(empty_bonus=0.5), dict(isect_cost=5, trav_cost=3),
                                dict(isect_cost=200, empty_bonus=0.2, max_prims=2)])
def test_non_default_parameters_equal_the_restatement(hprt, kw):
    rng = np.random.default_rng(7)
    lo, hi = _random_boxes(rng, 2500, flat=0.1, point=0.05, grid=0.25)
    _same_tree(hprt, lo, hi, **kw)


def test_three_triangle_tree_by_hand(hprt):
    """Boxes of three triangles along x: A [0,1], B [1.5,2.5], C [4,5] (y, z in [0,1]).  Root bounds [0,5] x [0,1]^2, SA 22.
    Split candidates on x (the edges strictly inside): t = 1: 1 + 80 (6*1 + 18*2) / 22; t = 1.5: 1 + 80 (8 + 16*2) / 22;
    t = 2.5: 1 + 80 (12*2 + 12*1) / 22 (best); t = 4: 1 + 80 (18*2 + 6) / 22.  y and z have no inner edges.  Above 2.5: C;
    below: A, B, bounds [0, 2.5]: t = 1 and t = 1.5 cost the same, the first wins.  Below child first (node + 1), then the
    above child; the root's above child is node 4."""
    lo = np.array([[0, 0, 0], [1.5, 0, 0], [4, 0, 0]], np.float32)
    hi = np.array([[1, 1, 1], [2.5, 1, 1], [5, 1, 1]], np.float32)
    t = hprt.KdTree.from_bounds(lo, hi)
    nodes, idx = t.arrays()
    want = np.array([[_f2u(2.5), 0 | 4 << 2], [_f2u(1.0), 0 | 3 << 2], [0, 3 | 1 << 2], [1, 3 | 1 << 2], [2, 3 | 1 << 2]], np.uint32)
    assert np.array_equal(nodes, want), nodes
    assert idx.shape == (0,)
    assert t.info() == {"nodes": 5, "leaves": 3, "prim_refs": 0, "depth": 2}


def _leaf_regions(nodes, idx, root_lo, root_hi):
    out = []
    stack = [(0, np.array(root_lo, np.float64), np.array(root_hi, np.float64), 0)]
    while stack:
        k, lo, hi, depth = stack.pop()
        a, b = int(nodes[k, 0]), int(nodes[k, 1])
        if b & 3 == 3:
            np_ = b >> 2
            prims = [] if np_ == 0 else [a] if np_ == 1 else idx[a:a + np_].tolist()
            out.append((lo, hi, set(prims), depth))
        else:
            ax = b & 3; s = struct.unpack("<f", struct.pack("<I", a))[0]
            lo1 = lo.copy(); hi0 = hi.copy()
            hi0[ax] = s; lo1[ax] = s
            stack.append((k + 1, lo, hi0, depth + 1))
            stack.append((b >> 2, lo1, hi, depth + 1))
    return out


@pytest.mark.parametrize("seed,kw", [(1, {}), (2, dict(max_prims=3)), (3, dict(max_depth=6))])
def test_structural_invariants(hprt, seed, kw):
    rng = np.random.default_rng(seed)
    lo, hi = _random_boxes(rng, 1500, flat=0.2, point=0.05)
    t = hprt.KdTree.from_bounds(lo, hi, **kw)
    nodes, idx = t.arrays()
    max_depth = kw.get("max_depth", round(2 + 1.6 * int(np.log2(lo.shape[0]))))
    for rlo, rhi, prims, depth in _leaf_regions(nodes, idx, lo.min(0), hi.max(0)):
        assert depth <= max_depth
        # every primitive whose box overlaps the leaf's region (with volume on the split axes) is listed in the leaf
        inside = np.all((lo < rhi) & (hi > rlo), axis=1)
        missing = set(np.nonzero(inside)[0].tolist()) - prims
        assert not missing, (rlo, rhi, sorted(missing)[:5])
    assert t.info()["depth"] <= max_depth


def test_front_end_parameters(hprt, tmp_path):
    from test_host_side import HEADER, _mesh_scene
    P = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 1], [3, 0, 1], [2, 1, 1]], np.float32)
    idx = np.arange(6, dtype=np.int32).reshape(2, 3)

    def parse(acc):
        p = tmp_path / "s.pbrt"
        p.write_text(_mesh_scene(P, idx).replace('Accelerator "bvh"', acc))
        return hprt.Model.parse(str(p))

    m = parse('Accelerator "kdtree"')
    assert m.accelerator == "kdtree"
    assert any("hprt_scene_attach_kdtree" in w for w in m.warnings())
    assert not any("outside the hot-path scope" in w for w in m.warnings())
    # defaults 80 / 1 / 0 / 1 / -1 give the tree from_bounds gives with its defaults
    lo = np.stack([P[0:3].min(0), P[3:6].min(0)]); hi = np.stack([P[0:3].max(0), P[3:6].max(0)])
    assert np.array_equal(hprt.KdTree(m).arrays()[0], hprt.KdTree.from_bounds(lo, hi).arrays()[0])
    # the statistics-only parameters are accepted without a warning; the others reach the builder
    m2 = parse('Accelerator "kdtree" "float splitalpha" [10] "integer alphatype" [1] "integer axisselectiontype" [2] '
               '"integer axisselectionamount" [3] "integer maxprims" [4] "integer maxdepth" [3] "integer intersectcost" [20] '
               '"integer traversalcost" [2] "float emptybonus" [0.5]')
    assert not any("not used" in w for w in m2.warnings()), m2.warnings()
    assert np.array_equal(hprt.KdTree(m2).arrays()[0], hprt.KdTree.from_bounds(lo, hi, 20, 2, 0.5, 4, 3).arrays()[0])
    assert parse('Accelerator "bvh"').accelerator == "bvh"
    assert hprt.Model.load(KILLEROO).accelerator == "bvh"


def test_depth_is_reported_and_bounded(hprt):
    """info()["depth"] is the interior levels of the deepest path (what the walk's todo list must hold); a full empty bonus
    makes every empty-space cut free, so the tree goes deep — and stays within maxdepth and the walk's capacity."""
    rng = np.random.default_rng(0)
    lo = rng.uniform(-10, 10, (3000, 3)).astype(np.float32); hi = (lo + rng.uniform(0.1, 2, (3000, 3))).astype(np.float32)
    for kw in (dict(), dict(empty_bonus=1.0, max_depth=48)):
        t, nodes, idx = _same_tree(hprt, lo, hi, **kw)
        depth = max(d for _, _, _, d in _leaf_regions(nodes, idx, lo.min(0), hi.max(0)))
        assert t.info()["depth"] == depth <= min(hprt.KD_MAX_DEPTH, kw.get("max_depth", 64))
    assert t.info()["depth"] > 30


def test_pixel_stats_files_of_a_kd_render(hprt, tmp_path):
    st = np.arange(3 * 4 * 7, dtype=np.uint64).reshape(3, 4, 7)
    hprt.write_pixel_stats_accel(str(tmp_path / "kd"), st, hprt.ACCEL_KDTREE)
    names = sorted(p.name for p in tmp_path.iterdir())
    assert names == sorted("kd-%s.txt" % n for n in ("primitiveIntersections", "primitiveIntersectionsP", "kdTreeNodeTraversals", "kdTreeNodeTraversalsP",
                                                   "bspTreeNodeTraversals", "bspTreeNodeTraversalsP", "leafNodeTraversals", "leafNodeTraversalsP"))
    assert np.array_equal(np.loadtxt(tmp_path / "kd-kdTreeNodeTraversals.txt", dtype=np.uint64), st[:, :, 5])
    assert np.array_equal(np.loadtxt(tmp_path / "kd-kdTreeNodeTraversalsP.txt", dtype=np.uint64), st[:, :, 6])
    assert np.array_equal(np.loadtxt(tmp_path / "kd-leafNodeTraversals.txt", dtype=np.uint64), st[:, :, 3])
    assert np.loadtxt(tmp_path / "kd-bspTreeNodeTraversals.txt").sum() == 0
    # the BVH form is what hprt_write_pixel_stats writes
    hprt.write_pixel_stats_accel(str(tmp_path / "bvh"), st, hprt.ACCEL_BVH)
    assert np.loadtxt(tmp_path / "bvh-kdTreeNodeTraversals.txt").sum() == 0
    with pytest.raises(hprt.HprtError):
        hprt.write_pixel_stats_accel(str(tmp_path / "x"), st, 7)
