"""The device Halton sampler held against the oracle's directly: halton_dim (csrc/device/dev_shading.h) through the probe kernel of
libhprt_probe.so over every dimension 0..999 and indices on both sides of 2^32 up to 2^63 - 1, in both forms a dimension has on the
device (the HBM tables; the workgroup's LDS copy k_shade reads dimensions below 64 from); whole paths whose Halton index lies
around and far above 2^32; and a render whose paths all run the 124 segments maxdepth 123 allows, through dimension 997.
Every comparison is bit for bit."""
import numpy as np
import pytest

import halton_cases as hc
from test_gpu_fuzz import COUNTERS

pytestmark = pytest.mark.gpu


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _mismatches(got, want, index, dim):
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    return "%d of %d differ; (dimension, index, device, oracle): %s" % (
        bad.size, got.size, [(int(dim[k]), int(index[k]), float(got[k]), float(want[k])) for k in bad[:8]])


# ---- a. every dimension ----

@pytest.fixture(scope="module")
def all_pairs():
    index, dim = hc.pairs(range(hc.N_DIMS), seed=21)
    low = np.bincount(dim[index < 2 ** 32], minlength=hc.N_DIMS)
    high = np.bincount(dim[index >= 2 ** 32], minlength=hc.N_DIMS)
    assert low.min() > 800 and high.min() > 100, "every dimension is probed on both sides of 2^32"
    assert (index >= 2 ** 62).sum() >= hc.N_DIMS and index.max() == 2 ** 63 - 1
    print("halton probe: %d pairs, %d below 2^32, %d at or above, %d at or above 2^62" % (index.size, low.sum(), high.sum(), (index >= 2 ** 62).sum()))
    return index, dim


def test_every_dimension_from_the_hbm_tables(orc, killeroo_scene, all_pairs):
    """radical_inverse_base over all 1,000 dimensions (primes up to 7,919, primeSums up to 3.68 M), about 1,300 indices each: the
    quotient by the 64-bit magic below 2^32, the 64-bit division above, (float) of a 64-bit reversedDigits."""
    index, dim = all_pairs
    assert index.size > 1200 * hc.N_DIMS
    bounds = hc.LAYOUTS["700x700"]
    want = orc.halton_dims(bounds, index, dim)
    got = killeroo_scene.debug_device_halton(700, 700, index, dim)
    assert _same(got, want), _mismatches(got, want, index, dim)
    assert np.unique(want).size > index.size // 2


@pytest.mark.parametrize("name", sorted(hc.LAYOUTS))
@pytest.mark.parametrize("center", [False, True])
def test_lds_form_against_the_oracle_and_the_hbm_form(orc, killeroo_scene, all_pairs, name, center):
    """Dimensions 0..63 through the LDS copy (scrambled_radical_inverse_lds: the 32-bit digit loop with its one-compare repair below
    2^32, its else branch above) and a few from 64 up, which fall through to the HBM tables; dimensions 0 and 1 under every layout
    and both sample_pixel_center values.  The two forms of one dimension must also agree with each other."""
    index, dim = all_pairs
    pick = (dim < hc.LDS_DIMS) | np.isin(dim, (64, 65, 333, 999))
    index, dim = index[pick], dim[pick]
    assert set(np.unique(dim).tolist()) == set(range(hc.LDS_DIMS)) | {64, 65, 333, 999}
    bounds = hc.LAYOUTS[name]
    w, h = bounds[2] - bounds[0], bounds[3] - bounds[1]
    want = orc.halton_dims(bounds, index, dim, center=center)
    lds = killeroo_scene.debug_device_halton(w, h, index, dim, sample_pixel_center=center, use_lds=True)
    hbm = killeroo_scene.debug_device_halton(w, h, index, dim, sample_pixel_center=center, use_lds=False)
    assert _same(lds, want), "LDS form: " + _mismatches(lds, want, index, dim)
    assert _same(hbm, want), "HBM form: " + _mismatches(hbm, want, index, dim)
    assert _same(lds, hbm)
    if center:
        assert (want[dim < 2] == 0.5).all()


def test_probe_refuses_a_dimension_outside_the_tables(hprt, killeroo_scene):
    for d in (-1, hc.N_DIMS):
        with pytest.raises(hprt.HprtError):
            killeroo_scene.debug_device_halton(700, 700, [5], [d])


# ---- b. whole paths across 2^32 ----

def _straddling_triples(rng, n, bounds, stride):
    px = rng.integers(bounds[0], bounds[2], n).astype(np.int32)
    py = rng.integers(bounds[1], bounds[3], n).astype(np.int32)
    return px, py, hc.straddling_samples(rng, n, stride)


def test_paths_with_indices_across_2_32(hprt, orc, killeroo_model, killeroo_scene, killeroo_oracle):
    """hprt_sample_radiance on the 700 x 700 killeroo frame (stride 31,104): half the samples in 138,083..138,086, where the pixel's
    offset decides on which side of 2^32 the index falls, half with an index about 2^e, e in [32, 62]."""
    opt = killeroo_model.options.copy()
    killeroo_oracle.set_film(crop=(0, 1, 0, 1), spp=opt.spp)
    n = 20000
    px, py, s = _straddling_triples(np.random.default_rng(31), n, (0, 0, 700, 700), 31104)
    index = np.array([orc.lib.orc_halton(0, 0, 700, 700, int(a), int(b), int(c), 0, 0, None) for a, b, c in zip(px, py, s)], np.uint64)
    tab, direct, bounds = hprt.debug_halton_index(opt, px, py, s)
    assert bounds == (0, 0, 700, 700) and np.array_equal(tab, index) and np.array_equal(direct, index)
    below, above = int((index < 2 ** 32).sum()), int((index >= 2 ** 32).sum())
    print("paths across 2^32: %d indices below, %d at or above, largest 2^%.2f" % (below, above, np.log2(float(index.max()))))
    assert below > 500 and above > 15000 and index.max() > 2 ** 61
    L0 = killeroo_oracle.sample_radiance(px, py, s)
    L1 = killeroo_scene.sample_radiance(px, py, s, opt)
    bad = np.any(L0.view(np.uint32) != L1.view(np.uint32), axis=1)
    assert not bad.any(), "%d of %d samples differ (%d of them below 2^32); max |d| = %g" % (
        int(bad.sum()), n, int((bad & (index < 2 ** 32)).sum()), float(np.abs(L0 - L1).max()))
    nonzero = float((L0.max(axis=1) > 0).mean())
    print("paths across 2^32: %.3f of the samples carry radiance" % nonzero)
    assert np.isfinite(L0).all() and nonzero > 0.8


# ---- c. every dimension in a render ----

def _quad(a, b, c, d):
    return 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [%s]\n' % "  ".join("%g %g %g" % p for p in (a, b, c, d))


# A closed room, x, y in [-4, 4], z in [0, 5]: floor, ceiling and three walls nearly white matte, the +x wall a mirror, a glass sphere
# and two point lights inside, the camera inside.  With rrthreshold 0 no path is cut by Russian roulette and nothing absorbs, so
# (nearly) every path runs all 124 segments of maxdepth 123 and draws dimension 5 + 8 * 124 = 997.
ROOM = ("""LookAt -3.2 -3.4 2.1  0.6 0.4 1.6  0 0 1
Camera "perspective" "float fov" [62]
Film "image" "integer xresolution" [24] "integer yresolution" [16]
Sampler "halton" "integer pixelsamples" [2]
Integrator "path" "integer maxdepth" [123] "float rrthreshold" [0]
WorldBegin
LightSource "point" "point from" [-1.5 1 4.2] "color I" [9 8.5 8]
LightSource "point" "point from" [2.5 -2.5 1.2] "color I" [3 4 5]
Material "matte" "color Kd" [.98 .97 .96]
""" + _quad((-4, -4, 0), (4, -4, 0), (4, 4, 0), (-4, 4, 0)) + _quad((-4, -4, 5), (-4, 4, 5), (4, 4, 5), (4, -4, 5)) +
        _quad((-4, -4, 0), (-4, -4, 5), (4, -4, 5), (4, -4, 0)) + _quad((-4, 4, 0), (4, 4, 0), (4, 4, 5), (-4, 4, 5)) +
        _quad((-4, -4, 0), (-4, 4, 0), (-4, 4, 5), (-4, -4, 5)) +
        'Material "mirror"\n' + _quad((4, -4, 0), (4, -4, 5), (4, 4, 5), (4, 4, 0)) +
        'AttributeBegin\nMaterial "glass"\nTranslate 1 .5 1.3\nShape "sphere" "float radius" [1.1]\nAttributeEnd\nWorldEnd\n')


@pytest.fixture(scope="module")
def room(hprt, orc, tmp_path_factory):
    d = tmp_path_factory.mktemp("room")
    p = d / "room.pbrt"
    p.write_text(ROOM)
    model = hprt.Model.parse(str(p))
    assert model.warnings() == [], model.warnings()
    baked = str(d / "room.hprt")
    model.save(baked)
    oracle = orc.OracleScene(baked)
    _, film, counters, _, _ = oracle.render(threads=8)
    return model, oracle, film, counters


def test_room_paths_run_to_the_last_dimension(room):
    """What keeps the render test below from passing emptily, on the oracle alone: (nearly) every path is 124 segments long, and the
    last bounce is visible in the film's bits."""
    model, oracle, film, c = room
    assert c["camera_rays"] == 24 * 16 * 2
    print("room: %d rays of %d" % (c["rays"], 124 * c["camera_rays"]))
    assert c["rays"] >= 0.99 * 124 * c["camera_rays"]
    oracle.set_film(max_depth=122)
    try:
        _, shorter, c122, _, _ = oracle.render(threads=8)
    finally:
        oracle.set_film(max_depth=123)
    moved = float(np.any(film.view(np.uint32) != shorter.view(np.uint32), axis=2).mean())
    print("room: maxdepth 122 moves %.4f of the pixels" % moved)
    assert c122["rays"] < c["rays"] and moved >= 0.9


def test_room_render_through_every_dimension(hprt, room):
    model, oracle, film0, c0 = room
    scene = hprt.Scene(model, hprt.Bvh(model))
    film1, st = scene.render(count_work=True)
    bad = np.any(film0.view(np.uint32) != film1.view(np.uint32), axis=2)
    assert not bad.any(), "%d pixels differ, max |d| = %g" % (int(bad.sum()), float(np.abs(film0 - film1).max()))
    for k in COUNTERS:
        assert st[k] == c0[k], (k, st[k], c0[k])
    plain, _ = scene.render()
    assert _same(plain, film0)
    scene.debug_poison(0xFF)
    try:
        poisoned, _ = scene.render()
    finally:
        scene.debug_poison(None)
    assert _same(poisoned, film0)


def test_room_samples_with_64_bit_indices(hprt, room):
    """Dimension 997 and an index above 2^32 in one path: the room's samples at the sample numbers of the killeroo case (24 x 16
    bounds: stride 32 * 27)."""
    model, oracle, _, _ = room
    opt = model.options.copy()
    stride = 32 * 27
    n = 2000
    px, py, s = _straddling_triples(np.random.default_rng(41), n, (0, 0, 24, 16), stride)
    tab, index, bounds = hprt.debug_halton_index(opt, px, py, s)
    assert bounds == (0, 0, 24, 16) and np.array_equal(tab, index)
    assert (index < 2 ** 32).sum() > 50 and (index >= 2 ** 32).sum() > 1400 and index.max() > 2 ** 61
    scene = hprt.Scene(model, hprt.Bvh(model))
    L0 = oracle.sample_radiance(px, py, s)
    L1 = scene.sample_radiance(px, py, s, opt)
    bad = np.any(L0.view(np.uint32) != L1.view(np.uint32), axis=1)
    assert not bad.any(), "%d of %d samples differ; max |d| = %g" % (int(bad.sum()), n, float(np.abs(L0 - L1).max()))
    assert np.isfinite(L0).all() and (L0.max(axis=1) > 0).mean() > 0.9
