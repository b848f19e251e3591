"""bsdf_sample_specular (csrc/device/dev_specular.h) — BSDF::Sample_f under the lobe masks of SpecularReflect and SpecularTransmit
(core/integrator.cpp:368, 411) — through a probe kernel of libhprt_probe.so against the oracle's lobe-array BSDF::Sample_f
(oracle/orc_shading.h) with the same mask, the BSDF built as DirectLightingIntegrator::Li builds it (tests/dl_reference.cpp: smooth
glass as two specular lobes).  Both masks, every material and every query family of tests/bsdf_cases.py: u[0] on both sides of every
k / m (the uber lobe choice falls at 1 / 2), grazing directions, wo.z == 0.  Every comparison is bit for bit, NaN against NaN as a
class."""
import numpy as np
import pytest

import bsdf_cases as bc
import dl_ref

pytestmark = pytest.mark.gpu
MASKS = {"reflect": dl_ref.MASK_REFLECT, "transmit": dl_ref.MASK_TRANSMIT}


@pytest.fixture(scope="module")
def palette(hprt, orc, tmp_path_factory):
    d = tmp_path_factory.mktemp("bsdf_specular_palette")
    model, _ = bc.build_palette(hprt, orc, d)
    return hprt.Scene(model, hprt.Bvh(model)), dl_ref.DlScene(str(d / "palette.hprt"))


@pytest.mark.parametrize("mask", sorted(MASKS))
@pytest.mark.parametrize("cls", bc.CLASSES)
def test_device_masked_sample_equals_the_oracles(palette, cls, mask):
    scene, ref = palette
    q = bc.queries(bc.by_class(cls))
    assert set(np.unique(q["family"]).tolist()) == set(range(len(bc.FAMILIES)))
    want = ref.bsdf_specular(MASKS[mask], q["shape"], q["frame9"], q["wo"], q["u"])
    got = scene.debug_device_bsdf_specular(MASKS[mask], q["shape"], q["frame9"], q["wo"], q["u"])
    bad, nans = bc.compare(got, want)
    lines = ["%s / %s: %d of %d queries differ" % (cls, mask, bad.size, got.shape[0])]
    for i in bad[:8]:
        lines.append("  %s / %s: frame %s wo %s u %s\n    device %s\n    oracle %s" % (
            bc.NAMES[q["shape"][i]], bc.FAMILIES[q["family"][i]], q["frame9"][i].tolist(), q["wo"][i].tolist(), q["u"][i].tolist(),
            ["%.9g" % v for v in got[i]], ["%.9g" % v for v in want[i]]))
    assert bad.size == 0, "\n".join(lines)
    live = (want[:, 6] > 0) & (want[:, 0:3] != 0).any(axis=1)
    print("%s / %s: %d queries, %d live samples, %d NaN-against-NaN words" % (cls, mask, got.shape[0], int(live.sum()), nans))
    # what can recurse and what cannot: mirror reflects; smooth glass and uber do both; everything else matches neither mask
    if cls == "mirror":
        assert live.any() == (mask == "reflect")
    elif cls in ("glass", "uber"):
        assert live.sum() >= 100
    else:
        assert not live.any() and (want[:, 7] == 0).all()
        nothing = np.array([0, 0, 0, 9, 9, 9, 0, 0], np.float32)      # black, wi untouched, pdf 0: no lobe matches (core/reflection.cpp:708-713)
        assert (got == nothing).all()


def test_both_uber_transmission_lobes_are_chosen(palette):
    """an uber BSDF with opacity below one and a non-black Kt offers two SpecularTransmission lobes (1 - opacity straight through,
    Kt refracting): u[0] below 1 / 2 takes the first, pdf 1 / 2 either way"""
    scene, ref = palette
    names = [n for n in bc.by_class("uber")]
    q = bc.queries(names)
    got = scene.debug_device_bsdf_specular(MASKS["transmit"], q["shape"], q["frame9"], q["wo"], q["u"])
    half = got[:, 6] == np.float32(0.5)
    assert half.any(), "no uber entry of the palette offers two transmission lobes"
    lo, hi = half & (q["u"][:, 0] < 0.5), half & (q["u"][:, 0] >= 0.5)
    assert lo.any() and hi.any()
    # the straight-through lobe leaves the direction alone (wi = -wo up to the round trip through the frame, which the skewed frames of
    # the "frames" family do not close); the refracting one bends it unless the entry's index is 1 (on the oracle: 89 % against 52 %)
    straight = np.abs(got[:, 3:6] + q["wo"]).max(axis=1) < 1e-5
    assert straight[lo].mean() > straight[hi].mean() + 0.25, (straight[lo].mean(), straight[hi].mean())


def test_probe_refusals(hprt, palette):
    scene, _ = palette
    q = {k: v[:4] for k, v in bc.queries(["matte"]).items()}
    assert scene.debug_device_bsdf_specular(MASKS["reflect"], q["shape"], q["frame9"], q["wo"], q["u"]).shape == (4, 8)
    for mask in (0, 31, 16):
        with pytest.raises(hprt.HprtError):
            scene.debug_device_bsdf_specular(mask, q["shape"], q["frame9"], q["wo"], q["u"])
    shape = q["shape"].copy()
    shape[1] = len(bc.PALETTE)
    with pytest.raises(hprt.HprtError):
        scene.debug_device_bsdf_specular(MASKS["reflect"], shape, q["frame9"], q["wo"], q["u"])
