"""The device BSDF held against the oracle's directly: bsdf_init, bsdf_f, bsdf_pdf and bsdf_sample (csrc/device/dev_shading.h) through
the probe kernel of libhprt_probe.so against ComputeScatteringFunctions and BSDF::f / Pdf / Sample_f (oracle/orc_shading.h), over the
palette and the query families of tests/bsdf_cases.py — every material, every family, five modes.  Every comparison is bit for
bit; where the oracle's value is NaN the device's must be NaN too, with any sign and payload (the default NaN of x86 and of gfx950
differ).  tests/test_bsdf_cases_host.py checks that the queries reach what they are meant to reach."""
import numpy as np
import pytest

import bsdf_cases as bc

pytestmark = pytest.mark.gpu
MODES = ("info", "f", "pdf", "sample non-specular", "sample all")


@pytest.fixture(scope="module")
def palette(hprt, orc, tmp_path_factory):
    model, oracle = bc.build_palette(hprt, orc, tmp_path_factory.mktemp("bsdf_palette"))
    return hprt.Scene(model, hprt.Bvh(model)), oracle


def _args(q):
    return q["shape"], q["frame9"], q["wo"], q["wi"], q["u"]


def _report(q, mode, got, want, bad):
    lines = ["mode %d (%s): %d of %d queries differ" % (mode, MODES[mode], bad.size, got.shape[0])]
    for i in bad[:8]:
        lines.append("  %s / %s: frame %s wo %s wi %s u %s\n    device %s\n    oracle %s" % (
            bc.NAMES[q["shape"][i]], bc.FAMILIES[q["family"][i]], q["frame9"][i].tolist(), q["wo"][i].tolist(), q["wi"][i].tolist(), q["u"][i].tolist(),
            ["%.9g" % v for v in got[i]], ["%.9g" % v for v in want[i]]))
    return "\n".join(lines)


@pytest.mark.parametrize("cls", bc.CLASSES)
def test_device_bsdf_equals_the_oracle(palette, cls):
    scene, oracle = palette
    q = bc.queries(bc.by_class(cls))
    assert set(np.unique(q["family"]).tolist()) == set(range(len(bc.FAMILIES)))
    failures, nans = [], 0
    for mode in range(5):
        want = oracle.bsdf_eval(mode, *_args(q))
        got = scene.debug_device_bsdf(mode, *_args(q))
        bad, nan_pairs = bc.compare(got, want)
        nans += nan_pairs
        if bad.size:
            failures.append(_report(q, mode, got, want, bad))
    print("%s: %d queries x 5 modes compared, %d NaN-against-NaN words" % (cls, q["shape"].size, nans))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("cls", bc.CLASSES)
def test_device_sample_agrees_with_itself(palette, cls):
    """On the device alone, over the random family's directions and sample values.

    Sample_f over the two flag sets: the same for every BSDF without a specular lobe (the reference picks among the same lobes).  For
    the BSDFs without a non-specular lobe (mirror, smooth glass, uber with specular lobes only, the black entries) the non-specular
    set matches nothing: black, pdf 0, no type, wi untouched (core/reflection.cpp:708-713), whatever Sample_f(BSDF_ALL) gives.

    bsdf_sample's tail is bsdf_f / bsdf_pdf restated, as the reference's is: for the wi of a live non-specular sample, bsdf_f
    reproduces the sample's f bit for bit, and bsdf_pdf its pdf — except where the picked lobe is a MicrofacetReflection, whose
    Sample_f takes its pdf from the SAMPLED half vector (core/reflection.cpp:415) while Pdf() normalises wo + wi again (:421).  The
    re-evaluation needs the sample's local wi back exactly, so this test uses the identity frame, where to_world and to_local are
    exact; in a general frame the round trip through the world rounds."""
    scene, _ = palette
    q = bc.queries(bc.by_class(cls))
    keep = q["family"] == bc.FAMILIES.index("random")
    q = {k: v[keep] for k, v in q.items()}
    q["frame9"] = bc.identity_frames(q["shape"].size)
    s3 = scene.debug_device_bsdf(3, *_args(q))
    s4 = scene.debug_device_bsdf(4, *_args(q))
    specular = {bc.SPECULAR_R, bc.SPECULAR_T}
    for name in bc.by_class(cls):
        k = bc.NAMES.index(name)
        e = bc.PALETTE[k]
        m = q["shape"] == k
        if e.ncomp == 0:
            nothing = np.array([0, 0, 0, 9, 9, 9, 0, 0], np.float32)      # black, wi untouched, pdf 0, no type
            assert (s3[m] == nothing).all(), (name, s3[m][:4].tolist())
        elif not (e.types & specular):
            bad, _ = bc.compare(s3[m], s4[m])
            assert bad.size == 0, (name, bad.size, s3[m][bad[:4]].tolist(), s4[m][bad[:4]].tolist())
    stype = s3[:, 7].astype(np.int32)
    live = np.isfinite(s3).all(axis=1) & (s3[:, 6] > 0) & (s3[:, 0:3] != 0).any(axis=1) & ((stype & 16) == 0)
    if cls not in ("mirror", "glass"):
        assert live.sum() >= 1000, (cls, int(live.sum()))
    n_pdf = 0
    if live.any():
        sel = np.flatnonzero(live)
        wi = np.ascontiguousarray(s3[sel, 3:6])
        f = scene.debug_device_bsdf(1, q["shape"][sel], q["frame9"][sel], q["wo"][sel], wi, q["u"][sel])
        pdf = scene.debug_device_bsdf(2, q["shape"][sel], q["frame9"][sel], q["wo"][sel], wi, q["u"][sel])
        names = [bc.NAMES[k] for k in q["shape"][sel]]
        bad_f = np.flatnonzero((f[:, 0:3].view(np.uint32) != s3[sel, 0:3].view(np.uint32)).any(axis=1))
        assert bad_f.size == 0, "f: %d of %d differ: %s" % (bad_f.size, sel.size, [(names[i], f[i, 0:3].tolist(), s3[sel[i]].tolist()) for i in bad_f[:8]])
        # every pick but a MicrofacetReflection's: diffuse, glossy transmission, and substrate's FresnelBlend (type 3)
        mtype = np.array([bc.PALETTE[k].mtype for k in q["shape"][sel]])
        exact = (stype[sel] != bc.GLOSSY_R) | (mtype == 3)
        n_pdf = int(exact.sum())
        bad_p = np.flatnonzero(exact & (pdf[:, 0].view(np.uint32) != s3[sel, 6].view(np.uint32)))
        assert bad_p.size == 0, "pdf: %d of %d differ: %s" % (bad_p.size, n_pdf, [(names[i], float(pdf[i, 0]), s3[sel[i]].tolist()) for i in bad_p[:8]])
    print("%s: %d live non-specular samples re-evaluated (f), %d of them with an exactly reproducible pdf" % (cls, int(live.sum()), n_pdf))


def test_probe_refusals(hprt, palette, tmp_path):
    scene, _ = palette
    q = {k: v[:4] for k, v in bc.queries(["matte"]).items()}
    assert scene.debug_device_bsdf(1, *_args(q)).shape == (4, 8)
    for bad_shape in (-1, len(bc.PALETTE)):
        shape = q["shape"].copy()
        shape[2] = bad_shape
        with pytest.raises(hprt.HprtError):
            scene.debug_device_bsdf(1, shape, q["frame9"], q["wo"], q["wi"], q["u"])
    for mode in (-1, 5):
        with pytest.raises(hprt.HprtError):
            scene.debug_device_bsdf(mode, *_args(q))
    empty = {k: v[:0] for k, v in q.items()}
    with pytest.raises(hprt.HprtError):
        scene.debug_device_bsdf(1, *_args(empty))
    # a shape whose Kd is an image texture: the probe passes bsdf_init no overrides
    bc.write_checks_pfm(str(tmp_path / "checks.pfm"))
    p = tmp_path / "textured.pbrt"
    p.write_text(bc.TEXTURED_PBRT % {"dir": str(tmp_path)})
    model = hprt.Model.parse(str(p))
    assert model.warnings() == [], model.warnings()
    textured = hprt.Scene(model, hprt.Bvh(model))
    shape = np.zeros(4, np.int32)
    with pytest.raises(hprt.HprtError):
        textured.debug_device_bsdf(1, shape, q["frame9"], q["wo"], q["wi"], q["u"])
