"""The Halton sampler without a GPU: the oracle's batched SampleDimension (orc_halton_dims, what tests/test_gpu_halton.py holds the
device against) against a plain Python model at the indices where a radical inverse can go wrong, and the two ways the library
forms a sample's Halton index — a render's per-axis offset tables and hprt_sample_radiance's direct offset — against the oracle's."""
import ctypes as C

import numpy as np
import pytest

import halton_cases as hc
from test_oracle_pins import HALTON_KAT


@pytest.fixture(scope="module")
def tables(orc):
    perms = np.zeros(3682913, np.uint16)
    assert orc.lib.orc_perm_table(perms.ctypes.data_as(C.c_void_p), perms.size) == perms.size
    pr = hc.primes()
    sums = np.concatenate([[0], np.cumsum(pr)[:-1]]).astype(np.int64)
    return perms, sums, pr


def _check(orc, tables, bounds, center, index, dim):
    perms, sums, pr = tables
    got = orc.halton_dims(bounds, index, dim, center=center)
    want = np.array([hc.model_sample_dimension(bounds, center, int(i), int(d), perms, sums, pr) for i, d in zip(index, dim)], np.float32)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, [(int(dim[k]), int(index[k]), float(got[k]), float(want[k])) for k in bad[:8]]
    return got


def test_known_answers_through_the_batched_entry(orc):
    for (px, py), s, index, vals in HALTON_KAT:
        want = np.array([np.float32(v) for v in vals.split()], np.float32)
        got = orc.halton_dims((0, 0, 700, 700), np.full(8, index, np.uint64), np.arange(8, dtype=np.int32))
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (px, py, s, got, want)
        assert orc.halton_dims((0, 0, 700, 700), [index, index], [0, 1], center=True).tolist() == [0.5, 0.5]


def test_scrambled_dimensions_against_the_python_model(orc, tables):
    """Dimensions 2..69 (every LDS dimension and the first past them), the deepest dimension a render of the suite reached before
    (333), its neighbour, and 500, 997, 998, 999: every hand-picked index and 75 random ones of each class, about 20,000 values."""
    dims = list(range(2, 70)) + [333, 334, 500, 997, 998, 999]
    index, dim = hc.pairs(dims, seed=11, n_random=75)
    assert index.size > 19000 and (index >= 2 ** 62).any()
    for d in dims:
        mine = index[dim == d]
        assert (mine < 2 ** 32).any() and (mine >= 2 ** 32).any()
    got = _check(orc, tables, hc.LAYOUTS["700x700"], False, index, dim)
    assert 0 <= got.min() and got.max() <= hc.ONE_MINUS_EPS and np.unique(got).size > got.size // 2


@pytest.mark.parametrize("name", sorted(hc.LAYOUTS))
@pytest.mark.parametrize("center", [False, True])
def test_dimensions_0_and_1_against_the_python_model(orc, tables, name, center):
    """Dimension 0 drops baseExponents[0] bits of the index and dimension 1 divides it by baseScales[1]: both depend on the layout, and
    with sample_pixel_center both are 0.5.  Dimension 2 rides along: no layout may move it."""
    index, dim = hc.pairs([0, 1, 2], seed=12, n_random=100)
    got = _check(orc, tables, hc.LAYOUTS[name], center, index, dim)
    if center:
        assert (got[dim < 2] == 0.5).all()
    else:
        assert np.unique(got[dim == 0]).size > 100 and np.unique(got[dim == 1]).size > 100
    assert np.array_equal(got[dim == 2], orc.halton_dims(hc.LAYOUTS["1x1"], index[dim == 2], dim[dim == 2]))


SIZES = (1, 2, 3, 16, 17, 100, 127, 128, 129, 700)
SAMPLES = (0, 1, 138084, 2 ** 40)


def _axis(lo, n):
    """pixels of [lo, lo + n): both ends, and the three pixels around every multiple of 128 inside"""
    hi = lo + n
    c = {lo, hi - 1}
    for k in range(0, hi + 128, 128):
        c |= {k - 1, k, k + 1}
    return sorted(v for v in c if lo <= v < hi)


@pytest.mark.parametrize("origin", [(0, 0), (127, 255), (300, 129)])
def test_index_parity_of_renders_and_sample_calls(hprt, orc, origin):
    """A render reads a pixel's offset from two 128-entry tables (SetupFrame: offX[x mod 128] + offY[y mod 128], reduced modulo the
    stride); hprt_sample_radiance computes it from the pixel.  Both, and the sample's term, against HaltonSampler::GetIndexForSample."""
    res = 1024
    checked = 0
    for w in SIZES:
        for h in SIZES:
            opt = hprt.RenderOptions()
            opt.xres = opt.yres = res
            opt.filter_radius[0] = opt.filter_radius[1] = 0.5
            x0, y0 = origin
            for i, v in enumerate((x0, x0 + w, y0, y0 + h)):
                opt.crop[i] = v / res                                   # (exact: res is a power of two)
            xs, ys = _axis(x0, w), _axis(y0, h)
            px, py, s = (a.ravel() for a in np.meshgrid(xs, ys, SAMPLES, indexing="ij"))
            tab, direct, bounds = hprt.debug_halton_index(opt, px, py, s)
            assert bounds == (x0, y0, x0 + w, y0 + h)
            want = np.array([orc.lib.orc_halton(*bounds, int(a), int(b), int(c), 0, 0, None) for a, b, c in zip(px, py, s)], np.uint64)
            assert np.array_equal(tab, want), (bounds, "offset tables")
            assert np.array_equal(direct, want), (bounds, "direct offset")
            checked += want.size
    assert checked > 5000      # (100 bounds, four sample numbers each at up to 17 x 17 pixels)


def test_index_hook_refuses_pixels_outside_the_bounds(hprt):
    opt = hprt.RenderOptions()
    opt.xres = opt.yres = 64
    opt.filter_radius[0] = opt.filter_radius[1] = 0.5
    opt.crop[1] = opt.crop[3] = 1.0
    hprt.debug_halton_index(opt, [63], [0], [5])
    for bad in (([64], [0], [0]), ([0], [-1], [0]), ([0], [0], [-1])):
        with pytest.raises(hprt.HprtError):
            hprt.debug_halton_index(opt, *bad)
