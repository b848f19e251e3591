"""The kd walk on the GPU (Accelerator "kdtree"): closest and any hit held bit for bit to the test-side restatement of
KdTreeAccel::Intersect / IntersectP (tests/kd_reference.cpp over tests/tree_reference.h) — t, primitive, barycentrics and all four
counters — on camera, random, degenerate and on-the-split-plane rays; renders against the reference's images; per-pixel
statistics; tile sharding; kernel resources.  The checks shared with the other tree walks are tests/tree_walk_checks.py's."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, KILLEROO
from tree_ref import kd as kd_ref
import tree_walk_checks as twc

pytestmark = pytest.mark.gpu
DODECA = os.path.join(GOLDEN, "dodecahedron.hprt")


@pytest.fixture(scope="module", params=[KILLEROO, DODECA], ids=["killeroo-simple", "dodecahedron"])
def kd(request, hprt, orc):
    path = request.param
    m = hprt.Model.load(path)
    sc = hprt.Scene(m, hprt.Bvh(m), device=0)
    sc.attach_kdtree(hprt.KdTree(m))
    return path, m, sc, kd_ref.KdScene(path), orc.OracleScene(path)


def _rays(ref, oracle, n, seed):
    rng = np.random.default_rng(seed)
    lo, hi = ref.bounds()
    blo, bhi = lo.min(0), hi.max(0)
    ext = bhi - blo
    out = [twc.camera_rays(rng, oracle, n), twc.random_rays(rng, blo, ext, n)]
    # zero direction components of either sign (1 / 0 = inf, 0 * inf = NaN), NaN / inf directions, rays aimed at primitives
    o = (blo + rng.uniform(-0.2, 1.2, (n, 3)) * ext).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    k = n // 8
    d[:k, 0] = 0.0; d[k:2 * k, 1] = -0.0; d[2 * k:3 * k, 0] = 0.0; d[2 * k:3 * k, 2] = -0.0
    d[3 * k:3 * k + 8] = np.nan; d[3 * k + 8:3 * k + 16, 1] = np.inf
    aim = rng.integers(0, lo.shape[0], 2 * k)
    d[4 * k:6 * k] = ((lo[aim] + hi[aim]) * np.float32(0.5) - o[4 * k:6 * k]).astype(np.float32)
    out.append((o, d, np.full(n, np.inf, np.float32)))
    # origins exactly on split planes (o[axis] == split: the belowFirst tie), directions of every sign along that axis
    ax, pos = ref.splits()
    pick = rng.integers(0, ax.shape[0], n)
    o = (blo + rng.uniform(0, 1, (n, 3)) * ext).astype(np.float32)
    o[np.arange(n), ax[pick]] = pos[pick]
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d[np.arange(n)[: n // 3], ax[pick][: n // 3]] = 0.0
    d[np.arange(n)[n // 3: n // 2], ax[pick][n // 3: n // 2]] = -0.0
    out.append((o, d, np.full(n, np.inf, np.float32)))
    return out


def test_closest_hit_equals_the_reference_walk(kd):
    _, _, sc, ref, oracle = kd
    twc.check_closest(sc, ref, _rays(ref, oracle, 20000, 1))


def test_any_hit_equals_the_reference_walk(kd):
    _, _, sc, ref, oracle = kd
    twc.check_any(sc, ref, _rays(ref, oracle, 20000, 2))


def test_device_entry_points_agree_with_the_host_ones(kd):
    _, _, sc, ref, oracle = kd
    twc.check_device_entry_points(sc, *_rays(ref, oracle, 4096, 3)[1])


def test_kd_renders_match_the_reference_images(hprt, kd):
    path, m, sc, _, _ = kd
    twc.check_reference_image(hprt, sc, m, path)


def test_counting_render_pixel_stats(hprt, kd, tmp_path):
    _, m, sc, _, _ = kd
    st, px, check_plain_film = twc.check_counting_render(sc, m)
    hprt.write_pixel_stats_accel(str(tmp_path / "kd"), px, hprt.ACCEL_KDTREE)
    assert np.array_equal(np.loadtxt(tmp_path / "kd-kdTreeNodeTraversals.txt", dtype=np.uint64).reshape(px.shape[:2]), px[:, :, 5])
    check_plain_film()


def test_tile_sharded_kd_render_merges_bit_identically(hprt, kd):
    _, m, sc, _, _ = kd
    twc.check_tile_sharding(hprt, sc, m)


def test_attach_refusals(hprt):
    m = hprt.Model.load(DODECA)
    sc = hprt.Scene(m, hprt.Bvh(m), device=0)
    rng = np.random.default_rng(0)
    lo = rng.uniform(0, 1, (7, 3)).astype(np.float32)
    with pytest.raises(hprt.HprtError) as e:
        sc.attach_kdtree(hprt.KdTree.from_bounds(lo, lo + 1))           # not this scene's primitive count
    assert e.value.code == hprt.E_INVALID
    mi = hprt.Model.load(os.path.join(GOLDEN, "simple_instanced.hprt"))
    si = hprt.Scene(mi, hprt.Bvh(mi), device=0)
    with pytest.raises(hprt.HprtError) as e:
        si.attach_kdtree(hprt.KdTree.from_bounds(lo[:1], lo[:1] + 1))
    assert e.value.code == hprt.E_UNSUPPORTED
    with pytest.raises(hprt.HprtError) as e:
        hprt.KdTree(mi)
    assert e.value.code == hprt.E_UNSUPPORTED


def test_kd_walk_resources(hprt, tmp_path):
    """Triangle-only kernels: <= 80 registers (six workgroups per CU), nothing in scratch; quadric kernels <= 128 (four);
    LDS: eight 8-byte todo entries per lane of a 256-thread workgroup."""
    twc.check_walk_resources(tmp_path, "k_kdwalk", 8 * 256 * 8)
