"""Integrator "directlighting", host side (no GPU needed): the front end's reading of the directive and of the lights' sample counts,
the test-side restatement (tests/dl_reference.cpp) held against the oracle's Halton sampler and against scenes whose direct lighting
is known, and the refusals of hprt_render_direct / hprt_sample_direct that are judged before a scene or a device is looked at."""
import ctypes as C

import numpy as np
import pytest

import dl_ref

SCENE = """LookAt 0 0 5  0 0 0  0 1 0
Camera "perspective" "float fov" [30]
Film "image" "integer xresolution" [%(xres)d] "integer yresolution" [%(yres)d] %(film)s
Sampler "halton" "integer pixelsamples" [%(spp)d]
%(integrator)s
WorldBegin
%(body)s
WorldEnd
"""
# a plane z = 0 facing the camera (which sits at z = 5), far larger than the view
QUAD = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-50 -50 %(z)s  50 -50 %(z)s  50 50 %(z)s  -50 50 %(z)s]'
PLANE = QUAD % dict(z="0")
NOTE = 'Integrator "directlighting": the host renders it with hprt_render_direct; hprt_render renders the path integrator'
DL = 'Integrator "directlighting"'


def _parse(hprt, d, name, integrator=DL, body='Material "matte"\n' + PLANE, xres=16, yres=16, spp=2, film=""):
    p = d / (name + ".pbrt")
    p.write_text(SCENE % dict(xres=xres, yres=yres, spp=spp, integrator=integrator, body=body, film=film))
    return hprt.Model.parse(str(p))


def _restated(hprt, d, name, **kw):
    m = _parse(hprt, d, name, **kw)
    path = str(d / (name + ".hprt"))
    m.save(path)
    s = dl_ref.DlScene(path)
    s.set_options(m.options)
    return m, s


# ---- front end ----
def test_defaults_and_note(hprt, tmp_path):
    m = _parse(hprt, tmp_path, "dl")
    assert m.direct() == ("all", 5, [])
    assert m.integrator() == ("directlighting", 64, True)      # hprt_model_integrator keeps its shape
    assert m.warnings() == [NOTE]


def test_strategy_one_maxdepth_and_pixelbounds(hprt, tmp_path):
    m = _parse(hprt, tmp_path, "dl", DL + ' "string strategy" ["one"] "integer maxdepth" [3] "integer pixelbounds" [0 4 0 4]')
    assert m.direct() == ("one", 3, [])
    assert m.warnings() == [NOTE]      # pixelbounds stays ignored, as for the other integrators
    assert m.options.max_depth == 5    # the path integrator's own default: "maxdepth" was read for this integrator, not for the baked options


def test_an_unknown_strategy_warns_as_the_reference_does(hprt, tmp_path):
    m = _parse(hprt, tmp_path, "dl", DL + ' "string strategy" ["some"]')
    assert m.direct()[0] == "all"
    assert m.warnings() == ['Strategy "some" for direct lighting unknown. Using "all".', NOTE]


def test_path_parameters_are_unused_under_directlighting(hprt, tmp_path):
    m = _parse(hprt, tmp_path, "dl", DL + ' "float rrthreshold" [0.5]')
    assert m.warnings() == ['Parameter "float rrthreshold" of Integrator not used', NOTE]


def test_samples_win_over_nsamples_light_by_light(hprt, tmp_path):
    body = ('LightSource "point" "point from" [0 0 3] "integer nsamples" [9]\n'
            'LightSource "distant" "integer samples" [9]\n'
            'LightSource "infinite" "integer nsamples" [4]\n'
            'LightSource "infinite" "integer nsamples" [4] "integer samples" [6]\n'
            'LightSource "infinite" "integer samples" [-2]\n'
            'Material "matte"\n' + PLANE + '\n'
            'AttributeBegin\nAreaLightSource "diffuse" "integer samples" [3]\n' + QUAD % dict(z="9") + '\nAttributeEnd\n'
            'AttributeBegin\nAreaLightSource "diffuse" "integer nsamples" [7]\nTranslate 0 0 7\nShape "sphere" "float radius" [0.5]\nAttributeEnd\n'
            'AttributeBegin\nAreaLightSource "diffuse"\nTranslate 3 0 7\nShape "sphere" "float radius" [0.5]\nAttributeEnd\n')
    m = _parse(hprt, tmp_path, "lights", body=body)
    # point and distant lights have no count of their own (1); a mesh emitter is one light per triangle
    assert m.direct() == ("all", 5, [1, 1, 4, 6, 1, 3, 3, 7, 1])
    assert m.warnings() == [NOTE]
    assert m.counts()["lights"] == 9


def test_a_baked_model_reports_the_defaults(hprt, tmp_path):
    body = 'LightSource "infinite" "integer nsamples" [4]\nMaterial "matte"\n' + PLANE
    a = _parse(hprt, tmp_path, "a", DL + ' "string strategy" ["one"] "integer maxdepth" [2]', body=body)
    b = _parse(hprt, tmp_path, "b", 'Integrator "path"', body=body.replace(' "integer nsamples" [4]', ""))
    a.save(str(tmp_path / "a.hprt")); b.save(str(tmp_path / "b.hprt"))
    assert (tmp_path / "a.hprt").read_bytes() == (tmp_path / "b.hprt").read_bytes()      # host side only, not baked
    assert a.direct() == ("one", 2, [4])
    assert hprt.Model.load(str(tmp_path / "a.hprt")).direct() == ("all", 5, [1])
    assert b.direct() == ("all", 5, [1]) and b.warnings() == []


# ---- the restatement against the oracle's sampler ----
def test_arrays_and_camera_samples_are_the_oracles(hprt, orc, tmp_path):
    """a cropped film whose sample bounds start at (12, 6); three lights with 1, 3 and 4 samples, maxdepth 2: twelve arrays over
    dimensions 5 .. 28, array a's entry j at GetIndexForSample(j); the plain dimensions go on at 29"""
    spp, depth, counts = 3, 2, [1, 3, 4]
    body = ('LightSource "point" "point from" [0 0 3]\nLightSource "infinite" "integer nsamples" [3]\nLightSource "infinite" "integer samples" [4]\n'
            'Material "matte"\n' + PLANE)
    m, s = _restated(hprt, tmp_path, "crop", body=body, xres=40, yres=30, spp=spp, film='"float cropwindow" [0.3 0.8 0.2 0.9]')
    assert m.direct()[2] == counts
    (cx0, cy0, cx1, cy1), sb = s.bounds()
    assert (cx0, cy0) == (12, 6) and sb[:2] == [12, 6]
    for px, py in [(12, 6), (19, 11), (31, 26)]:
        arrays, cam, dim = s.pixel_samples(px, py, "all", depth, counts, spp)
        assert [a.shape[0] for a in arrays] == [spp * c for _ in range(depth) for c in counts for _ in range(2)]
        for a, u in enumerate(arrays):
            idx = np.array([orc.halton(sb, px, py, j, 5, 2)[0] for j in range(u.shape[0])], np.uint64)      # GetIndexForSample(j)
            want = np.stack([orc.halton_dims(sb, idx, np.full(idx.size, 5 + 2 * a, np.int32)), orc.halton_dims(sb, idx, np.full(idx.size, 6 + 2 * a, np.int32))], 1)
            assert np.array_equal(u.view(np.uint32), want.view(np.uint32)), (px, py, a)
        assert (dim == 5 + 4 * depth * len(counts)).all()
        for k in range(spp):
            index, head = orc.halton(sb, px, py, k, 0, 5)
            assert np.array_equal(cam[k, :5].view(np.uint32), head.view(np.uint32))      # Get2D's skip test at dimension 3 is false
            tail = orc.halton_dims(sb, np.full(2, index, np.uint64), np.array([dim[k], dim[k] + 1], np.int32))
            assert np.array_equal(cam[k, 5:].view(np.uint32), tail.view(np.uint32))
        # strategy "one" requests nothing: the plain dimensions go on at 5
        arrays1, cam1, dim1 = s.pixel_samples(px, py, "one", depth, counts, spp)
        assert arrays1 == [] and (dim1 == 5).all() and np.array_equal(cam1[:, :5].view(np.uint32), cam[:, :5].view(np.uint32))


# ---- the restatement against known answers ----
POINT = 'LightSource "point" "point from" [0 0 3] "color I" [10 8 6]\nMaterial "matte" "color Kd" [0.5 0.4 0.3]\n' + PLANE


def test_all_and_one_agree_on_a_delta_light(hprt, tmp_path):
    """one point light over a matte plane: a delta light reads no sample value, one light is picked whatever Get1D returns, and
    EstimateDirect / (1 / 1) is EstimateDirect: bit for bit"""
    m, s = _restated(hprt, tmp_path, "point", body=POINT, spp=3)
    fa, ca, La = s.render("all", 3)
    fo, co, Lo = s.render("one", 3)
    assert np.array_equal(fa.view(np.uint32), fo.view(np.uint32)) and np.array_equal(La.view(np.uint32), Lo.view(np.uint32))
    assert fa[..., :3].min() > 0
    assert ca["rays"] == co["rays"] == ca["camera_rays"] == 16 * 16 * 3 == ca["shadow_rays"] == co["shadow_rays"]
    assert ca["nodes_deep"] == 0


def test_a_point_light_over_a_plane_is_kd_i_cos_over_pi_d2(hprt, tmp_path):
    """every sample against Kd / pi * I * cos(theta) / d^2 in float64, the hit point from the sample's film position (the light sits on
    the camera's axis, so only the hit's distance from the axis enters).
    Measured over the window from the restatement: largest relative error 3.02e-6; the tolerance is four times that, 1.21e-5 (the
    float roundings of the raster-to-camera matrix, the camera ray, the hit point, Sample_Li and f * Li * |cos| / pdf; the hit's
    distance from the axis enters d^2 and the cosine, so an error of the ray's direction is felt three times)."""
    spp = 4
    m, s = _restated(hprt, tmp_path, "point", body=POINT, spp=spp)
    film, c, L = s.render("all", 1)
    worst = 0.0
    t = np.tan(np.radians(15.0))
    for py in range(16):
        for px in range(16):
            _, cam, _ = s.pixel_samples(px, py, "all", 1, None, spp)
            for k in range(spp):
                fx, fy = float(np.float32(px) + cam[k, 0]), float(np.float32(py) + cam[k, 1])      # (Float)px + u, as GetCameraSample forms it
                r2 = (5 * t) ** 2 * ((fx / 8 - 1) ** 2 + (1 - fy / 8) ** 2)
                d2 = r2 + 9.0
                want = np.array([0.5 * 10, 0.4 * 8, 0.3 * 6]) / np.pi * (3 / np.sqrt(d2)) / d2
                worst = max(worst, float((np.abs(L[k, py, px].astype(np.float64) - want) / want).max()))
    print("point light over a plane: largest relative error %.3g (tolerance 1.21e-5)" % worst)
    assert worst <= 1.21e-5


MIRROR = ('Material "mirror" "color Kr" [0.9 0.9 0.9]\n' + PLANE + '\nMaterial "matte" "color Kd" [0 0 0]\n'
          'AttributeBegin\nAreaLightSource "diffuse" "color L" [2 3 4] "bool twosided" ["true"]\n' + QUAD % dict(z="8") + '\nAttributeEnd\n')


def test_a_mirror_facing_an_emitter_returns_kr_le(hprt, tmp_path):
    """the camera looks at a Kr = 0.9 mirror; every reflected ray ends on a black-bodied emitter behind the camera.  A mirror has no
    non-specular lobe, so its own direct lighting is zero and L = f * Le * |cos| / pdf with f = Kr / |cos|, pdf = 1.
    Measured from the restatement: largest relative error 7.06e-8 (the quotient and the product by |cos| do not cancel exactly); the
    tolerance is four times that, 2.83e-7.  With maxdepth 1 nothing recurses: exactly zero."""
    m, s = _restated(hprt, tmp_path, "mirror", body=MIRROR, spp=2)
    film, c, L = s.render("all", 2)
    want = 0.9 * np.array([2.0, 3.0, 4.0])
    rel = float((np.abs(L.astype(np.float64) - want) / want).max())
    print("mirror facing an emitter: largest relative error %.3g (tolerance 2.83e-7)" % rel)
    assert rel <= 2.83e-7
    assert c["nodes_deep"] == 16 * 16 * 2 and c["samples_deep2"] == 0
    film1, c1, L1 = s.render("all", 1)
    assert (L1 == 0).all() and (film1[..., :3] == 0).all() and c1["nodes_deep"] == 0
    # strategy "one" on the way: the same tree, other dimensions
    film2, c2, L2 = s.render("one", 2)
    assert float((np.abs(L2.astype(np.float64) - want) / want).max()) <= 2.83e-7 and c2["nodes_deep"] == c["nodes_deep"]


def test_a_plane_under_a_constant_sky_is_kd_l_on_average(hprt, tmp_path):
    """a lone grey plane under a constant infinite light sampled four times per hit: E[L] = Kd * L (the irradiance of a constant sky is
    pi L); the mean over the film's samples lies within three of its own standard errors, formed from the restatement's per-sample
    values — a Monte-Carlo bound, not a device tolerance"""
    body = 'LightSource "infinite" "color L" [1 1 1] "integer nsamples" [4]\nMaterial "matte" "color Kd" [0.5 0.5 0.5]\n' + PLANE
    m, s = _restated(hprt, tmp_path, "sky", body=body, spp=4)
    assert m.direct()[2] == [4]
    film, c, L = s.render("all", 1, [4])
    v = L[..., 0].astype(np.float64).ravel()
    mean, se = v.mean(), v.std(ddof=1) / np.sqrt(v.size)
    print("constant sky: mean %.5f, standard error %.5f (%d samples)" % (mean, se, v.size))
    assert abs(mean - 0.5) <= 3 * se
    assert c["shadow_rays"] > 0 and c["rays"] > c["camera_rays"]      # both halves of EstimateDirect ran


GLASS = ('LightSource "point" "point from" [0 3 4] "color I" [10 10 10]\nMaterial "matte"\n' + QUAD % dict(z="-2") + '\n'
         'Material "glass" %s\nShape "sphere" "float radius" [1]\n')


def test_smooth_glass_recurses_through_two_lobes_and_rough_glass_does_not(hprt, tmp_path):
    """DirectLightingIntegrator::Li asks for the scattering functions without allowMultipleLobes (directlighting.cpp:75,
    core/interaction.h:132): smooth glass is then a SpecularReflection and a SpecularTransmission lobe (materials/glass.cpp:62-90), each
    matching one mask — not the FresnelSpecular lobe of the path integrator, which matches neither.  Rough glass has glossy lobes only."""
    m, s = _restated(hprt, tmp_path, "glass", body=GLASS % "", spp=2)
    film, c, L = s.render("all", 3)
    assert c["nodes_deep"] > 0 and c["samples_deep2"] > 0
    film1, c1, L1 = s.render("all", 1)
    assert c1["nodes_deep"] == 0
    m, s = _restated(hprt, tmp_path, "roughglass", body=GLASS % '"float uroughness" [0.2] "float vroughness" [0.2]', spp=2)
    film, c, L = s.render("all", 3)
    assert c["nodes_deep"] == 0


# ---- refusals: judged before the scene and the device ----
def _refusal(hprt, fn, strategy=0, max_depth=5, counts=None, spp=4, flags=0):
    opt = hprt.RenderOptions()
    opt.xres = opt.yres = 16
    opt.spp = spp
    dp = hprt.DirectParams(strategy, max_depth)
    c = None if counts is None else np.ascontiguousarray(counts, np.int32)
    cp, n = (None, 0) if c is None else (c.ctypes.data_as(C.c_void_p), c.shape[0])
    if fn == "render":
        desc = hprt.RenderDesc()
        desc.opt = opt
        desc.tile_stride, desc.flags = 1, flags
        rc = hprt.lib.hprt_render_direct(None, C.byref(desc), C.byref(dp), cp, n, None, None, None)
    else:
        rc = hprt.lib.hprt_sample_direct(None, C.byref(opt), C.byref(dp), cp, n, 0, None, None, None, None)
    return rc, hprt.lib.hprt_last_error().decode()


def _not_refused(hprt, rc, msg, word):
    """past the parameter checks: no scene was passed (or no device is there)"""
    assert rc in (hprt.E_INVALID, hprt.E_NO_DEVICE) and word not in msg, (rc, msg)


@pytest.mark.parametrize("fn", ["render", "sample"])
def test_depths_below_one_and_counts_below_one_are_invalid(hprt, fn):
    for d in (0, -2):
        rc, msg = _refusal(hprt, fn, max_depth=d)
        assert rc == hprt.E_INVALID and "max_depth must be at least 1" in msg, (d, rc, msg)
    for counts in ([0], [3, -1, 2]):
        rc, msg = _refusal(hprt, fn, counts=counts)
        assert rc == hprt.E_INVALID and "sample count must be at least 1" in msg, (counts, rc, msg)
    rc, msg = _refusal(hprt, fn, strategy=2)
    assert rc == hprt.E_INVALID and "strategy" in msg


@pytest.mark.parametrize("fn", ["render", "sample"])
def test_a_depth_above_the_cap_is_unsupported(hprt, fn):
    assert hprt.DIRECT_MAX_DEPTH >= 8
    rc, msg = _refusal(hprt, fn, max_depth=hprt.DIRECT_MAX_DEPTH + 1)
    assert rc == hprt.E_UNSUPPORTED and "max_depth above %d" % hprt.DIRECT_MAX_DEPTH in msg, (rc, msg)
    rc, msg = _refusal(hprt, fn, max_depth=hprt.DIRECT_MAX_DEPTH)      # no lights: 5 + 4 * 127 dimensions
    _not_refused(hprt, rc, msg, "max_depth above")


@pytest.mark.parametrize("fn", ["render", "sample"])
def test_a_tree_that_could_pass_1000_dimensions_is_unsupported(hprt, fn):
    # "one", depth 7: 5 + 5 * 127 + 4 * 63 = 892; depth 8: 5 + 5 * 255 + 4 * 127 = 1788
    rc, msg = _refusal(hprt, fn, strategy=1, max_depth=8, counts=[1])
    assert rc == hprt.E_UNSUPPORTED and "1,000 sampler dimensions" in msg, (rc, msg)
    rc, msg = _refusal(hprt, fn, strategy=1, max_depth=7, counts=[1])
    _not_refused(hprt, rc, msg, "1,000")
    # "all", depth 5, n lights: 5 + 20 n + 4 n * 26 + 60 = 65 + 124 n: 7 lights 933, 8 lights 1057
    rc, msg = _refusal(hprt, fn, max_depth=5, counts=[1] * 8)
    assert rc == hprt.E_UNSUPPORTED and "1,000 sampler dimensions" in msg, (rc, msg)
    rc, msg = _refusal(hprt, fn, max_depth=5, counts=[1] * 7)
    _not_refused(hprt, rc, msg, "1,000")


@pytest.mark.parametrize("fn", ["render", "sample"])
def test_an_overflowing_array_size_is_unsupported(hprt, fn):
    rc, msg = _refusal(hprt, fn, max_depth=1, counts=[1, 1024], spp=1 << 21)          # 2^31 = INT32_MAX + 1
    assert rc == hprt.E_UNSUPPORTED and "INT32_MAX" in msg, (rc, msg)
    rc, msg = _refusal(hprt, fn, max_depth=1, counts=[1, 1023], spp=1 << 21)
    _not_refused(hprt, rc, msg, "INT32_MAX")
    rc, msg = _refusal(hprt, fn, strategy=1, max_depth=1, counts=[1, 1024], spp=1 << 21)      # "one" requests no array
    _not_refused(hprt, rc, msg, "INT32_MAX")
    rc, msg = _refusal(hprt, fn, max_depth=1, counts=[40000, 40000])
    assert rc == hprt.E_UNSUPPORTED and "65,536" in msg, (rc, msg)


def test_flags_other_than_count_work_are_unsupported(hprt):
    for flag in (hprt.RENDER_PIXEL_STATS, hprt.RENDER_COUNT_TRACED, hprt.RENDER_TRACE_ALL, hprt.RENDER_EXPORT_FOREIGN, hprt.RENDER_COUNT_WORK | hprt.RENDER_TRACE_ALL):
        rc, msg = _refusal(hprt, "render", flags=flag)
        assert rc == hprt.E_UNSUPPORTED and "only HPRT_RENDER_COUNT_WORK" in msg, (flag, rc, msg)
    rc, msg = _refusal(hprt, "render", flags=hprt.RENDER_COUNT_WORK)
    _not_refused(hprt, rc, msg, "HPRT_RENDER_COUNT_WORK")


def test_the_entry_points_are_exported(hprt):
    for name in ("hprt_model_direct", "hprt_render_direct", "hprt_sample_direct"):
        assert name in hprt.EXPORTS
