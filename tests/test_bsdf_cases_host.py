"""The input conditions of tests/test_gpu_bsdf.py, checked on the oracle alone: the palette holds the materials it says it holds, every
query family reaches every material, and the queries reach the lobes, the picks and the dead ends the comparison is meant to cover —
so that the GPU test cannot pass by comparing nothing.  The floors are conditions on the generator (tests/bsdf_cases.py)."""
import numpy as np
import pytest

import bsdf_cases as bc


@pytest.fixture(scope="module")
def palette(hprt, orc, tmp_path_factory):
    return bc.build_palette(hprt, orc, tmp_path_factory.mktemp("bsdf_palette"))


@pytest.fixture(scope="module")
def q():
    return bc.queries()


@pytest.fixture(scope="module")
def sampled(palette, q):
    """mode 4 (Sample_f over BSDF_ALL) of every query, computed once"""
    return palette[1].bsdf_eval(4, q["shape"], q["frame9"], q["wo"], q["wi"], q["u"])


def _rows(q, k, family=None):
    m = q["shape"] == k
    if family is not None:
        m &= q["family"] == bc.FAMILIES.index(family)
    return m


def test_generator_bounds(q):
    n = q["shape"].size
    print("bsdf queries: %d over %d palette entries" % (n, len(bc.PALETTE)))
    assert n <= 2 ** 20 and 38 <= len(bc.PALETTE) <= 48
    assert q["u"].min() >= 0 and q["u"].max() < 1
    for k in ("frame9", "wo", "wi", "u"):
        assert np.isfinite(q[k]).all(), k
    zero_wh = np.zeros(n, bool)      # the refract family's wo + eta * wi == 0 queries: |wi| = 1 / eta (or eta)
    for k, e in enumerate(bc.PALETTE):
        m = _rows(q, k, "refract")
        for ep in (e.eta, np.float32(1) / e.eta):
            zero_wh |= m & np.all((q["wo"] + q["wi"] * ep).astype(np.float32) == 0, axis=1)
    assert zero_wh.sum() >= 100 * len(bc.PALETTE)
    length = lambda v: np.linalg.norm(v.astype(np.float64), axis=1)
    assert np.abs(length(q["wo"]) - 1).max() < 1e-3
    assert np.abs(length(q["wi"])[~zero_wh] - 1).max() < 1e-3
    assert np.abs(length(q["frame9"][:, 0:3]) - 1).max() < 1e-3 and np.abs(length(q["frame9"][:, 3:6]) - 1).max() < 1e-3
    d = length(q["frame9"][:, 6:9])
    frames = q["family"] == bc.FAMILIES.index("frames")
    assert np.abs(d[~frames] - 1).max() < 1e-3 and d[frames].min() >= .25 - 1e-3 and d[frames].max() <= 4 + 1e-3


def test_every_family_reaches_every_entry(q):
    for k, e in enumerate(bc.PALETTE):
        for fam in bc.FAMILIES:
            assert _rows(q, k, fam).sum() > 0, (e.name, fam)


def test_frames_family_splits_geometric_and_shading_sides(q):
    """dot(w, ng) and the local z (dot(w, ns)) differ in sign in a good share of the `frames` queries: BSDF::f's `reflect` and
    SameHemisphere then disagree"""
    m = q["family"] == bc.FAMILIES.index("frames")
    fr = q["frame9"][m].astype(np.float64)
    for w in (q["wo"][m].astype(np.float64), q["wi"][m].astype(np.float64)):
        differ = np.sign(np.sum(w * fr[:, 0:3], axis=1)) != np.sign(np.sum(w * fr[:, 3:6], axis=1))
        print("frames: %.3f of the directions lie between the two horizons" % differ.mean())
        assert differ.mean() > .15


def test_palette_materials_and_components(palette, q):
    """mode 0: material type, NumComponents(BSDF_ALL & ~BSDF_SPECULAR) and BSDF::eta of every entry, against the values written beside
    the entry in the palette"""
    _, oracle = palette
    first = np.array([np.flatnonzero(q["shape"] == k)[0] for k in range(len(bc.PALETTE))])
    info = oracle.bsdf_eval(0, q["shape"][first], q["frame9"][first], q["wo"][first], q["wi"][first], q["u"][first])
    for k, e in enumerate(bc.PALETTE):
        assert (int(info[k, 0]), int(info[k, 1])) == (e.mtype, e.ncomp), (e.name, info[k])
    eta = {e.name: float(info[k, 2]) for k, e in enumerate(bc.PALETTE)}
    # BSDF::eta: the glass index (materials/glass.cpp:53); uber's index only without a straight-through lobe (materials/uber.cpp:56-62)
    assert eta["glass_133"] == float(np.float32(1.33)) and eta["glass_kt_black"] == 3 and eta["roughglass"] == 1.5
    assert eta["uber_opaque"] == float(np.float32(1.4)) and eta["uber_all"] == 1 and eta["uber_kr_kt"] == float(np.float32(1.33))
    assert all(eta[e.name] == 1 for e in bc.PALETTE if e.mtype not in (5, 6))


def _live(out):
    return np.isfinite(out).all(axis=1) & (out[:, 6] > 0) & (out[:, 0:3] != 0).any(axis=1)


def test_random_family_is_mostly_live(palette, q, sampled):
    for k, e in enumerate(bc.PALETTE):
        live = _live(sampled[_rows(q, k, "random")])
        print("%-20s live %.3f" % (e.name, live.mean()))
        if e.has_lobe:
            assert live.mean() >= .5, (e.name, live.mean())
        else:
            assert not live.any(), e.name


def test_every_sampled_type_appears(palette, q, sampled):
    for k, e in enumerate(bc.PALETTE):
        out = sampled[_rows(q, k)]
        seen = {int(t) for t in np.unique(out[:, 7])} - {-1, 0}
        assert seen == set(e.types), (e.name, sorted(seen), sorted(e.types))
    # uber with every lobe: five picks, of which the straight-through lobe (wi = -wo: etaB = 1) and Kt (refracted) both report
    # specular transmission
    for name in ("uber_all",):
        k = bc.NAMES.index(name)
        m = _rows(q, k) & (sampled[:, 7] == bc.SPECULAR_T)
        straight = np.abs(sampled[m, 3:6] + q["wo"][m]).max(axis=1) < 1e-5
        print("%s: %d straight-through picks, %d Kt picks" % (name, straight.sum(), (~straight).sum()))
        assert straight.sum() >= 100 and (~straight).sum() >= 100


def test_dead_ends_are_reached(palette, q, sampled):
    for k, e in enumerate(bc.PALETTE):
        out = sampled[_rows(q, k)]
        untouched = (out[:, 6] == bc.SENTINEL_PDF) & (out[:, 7] == -1) & (out[:, 3:6] == 9).all(axis=1)
        failed = (out[:, 6] == 0) & (out[:, 7] == 0)
        print("%-20s pdf untouched %5d, pdf == 0 with no type %5d" % (e.name, untouched.sum(), failed.sum()))
        if e.has_lobe:
            assert untouched.sum() >= 100, e.name      # wo.z == 0
        else:
            assert failed.all(), e.name                # no matching lobe: nothing else can happen
        # a refraction that can fail (e.dead), or a microfacet reflection that can leave wo's hemisphere (every glossy reflection lobe)
        if e.dead or bc.GLOSSY_R in e.types:
            assert failed.sum() >= 100, e.name
        if e.smooth:
            # total internal reflection: from inside beyond the critical angle (identity frame: the local wo is wo)
            m = _rows(q, k, "refract")
            wo = q["wo"][m].astype(np.float64)
            tir = (wo[:, 2] < 0) & (np.sqrt(wo[:, 0] ** 2 + wo[:, 1] ** 2) * float(e.eta) > 1 + 1e-5)
            assert tir.sum() >= 100, (e.name, tir.sum())
            assert (sampled[m][tir, 7] == bc.SPECULAR_R).all() and (sampled[m][tir, 6] == 1).all(), e.name


def test_nan_only_where_expected(palette, q):
    _, oracle = palette
    allowed = np.isin(q["family"], [bc.FAMILIES.index("refract"), bc.FAMILIES.index("grazing")])
    total = 0
    for mode in range(5):
        out = oracle.bsdf_eval(mode, q["shape"], q["frame9"], q["wo"], q["wi"], q["u"])
        nan = np.isnan(out).any(axis=1)
        total += int(nan.sum())
        bad = np.flatnonzero(nan & ~allowed)
        assert bad.size == 0, "mode %d: %d NaN rows outside refract / grazing, first: %s" % (
            mode, bad.size, [(bc.NAMES[q["shape"][i]], bc.FAMILIES[q["family"][i]], q["wo"][i].tolist(), q["wi"][i].tolist(), q["u"][i].tolist(), out[i].tolist()) for i in bad[:4]])
    print("NaN rows over the five modes: %d" % total)
    assert total > 0      # the zero-half-vector refraction queries produce them
