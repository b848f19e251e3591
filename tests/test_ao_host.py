"""Integrator "ambientocclusion", host side (no GPU needed): the front end's reading of the directive, the test-side restatement
(tests/ao_reference.cpp) held against the oracle's Halton sampler and against geometry whose ambient occlusion is known, and the
refusals of hprt_render_ao / hprt_sample_ao, which are judged before a device is looked for."""
import ctypes as C

import numpy as np
import pytest

import ao_ref

SCENE = """LookAt 0 0 5  0 0 0  0 1 0
Camera "perspective" "float fov" [30]
Film "image" "integer xresolution" [%(xres)d] "integer yresolution" [%(yres)d] %(film)s
Sampler "halton" "integer pixelsamples" [%(spp)d]
%(integrator)s
WorldBegin
Material "matte"
%(body)s
WorldEnd
"""
# a lone plane z = 0 facing the camera, far larger than the view
PLANE = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-50 -50 0  50 -50 0  50 50 0  -50 50 0]'
# a closed box around the camera (which sits at z = 5): every hemisphere ray from a wall ends on another wall
BOX = ('Shape "trianglemesh" "integer indices" [0 1 2 0 2 3  4 6 5 4 7 6  0 4 5 0 5 1  1 5 6 1 6 2  2 6 7 2 7 3  3 7 4 3 4 0] '
       '"point P" [-4 -4 -1  4 -4 -1  4 4 -1  -4 4 -1  -4 -4 8  4 -4 8  4 4 8  -4 4 8]')
NOTE = 'Integrator "ambientocclusion": the host renders it with hprt_render_ao; hprt_render renders the path integrator'


def _parse(hprt, d, name, integrator, body=PLANE, xres=16, yres=16, spp=2, film=""):
    p = d / (name + ".pbrt")
    p.write_text(SCENE % dict(xres=xres, yres=yres, spp=spp, integrator=integrator, body=body, film=film))
    return hprt.Model.parse(str(p))


def _restated(hprt, d, name, **kw):
    m = _parse(hprt, d, name, 'Integrator "ambientocclusion"', **kw)
    path = str(d / (name + ".hprt"))
    m.save(path)
    s = ao_ref.AoScene(path)
    s.set_options(m.options)
    return m, s


# ---- front end ----
def test_defaults_and_note(hprt, tmp_path):
    m = _parse(hprt, tmp_path, "ao", 'Integrator "ambientocclusion"')
    assert m.integrator() == ("ambientocclusion", 64, True)
    assert m.warnings() == [NOTE]


def test_given_parameters_are_read_and_not_reported(hprt, tmp_path):
    m = _parse(hprt, tmp_path, "ao", 'Integrator "ambientocclusion" "integer nsamples" [7] "bool cossample" ["false"] "integer pixelbounds" [0 4 0 4]')
    assert m.integrator() == ("ambientocclusion", 7, False)
    assert m.warnings() == [NOTE]      # neither nsamples nor cossample "not used"; pixelbounds stays ignored, as for "path"


def test_path_parameters_are_unused_under_ao(hprt, tmp_path):
    m = _parse(hprt, tmp_path, "ao", 'Integrator "ambientocclusion" "integer maxdepth" [3] "float rrthreshold" [0.5] "integer nsamples" [4]')
    assert m.integrator() == ("ambientocclusion", 4, True)
    assert m.warnings() == ['Parameter "integer maxdepth" of Integrator not used', 'Parameter "float rrthreshold" of Integrator not used', NOTE]
    assert m.options.max_depth == 5      # CreatePathIntegrator's default: the directive's value was not read


def test_other_integrators_keep_their_warning(hprt, tmp_path):
    m = _parse(hprt, tmp_path, "w", 'Integrator "whitted"')
    assert m.warnings() == ['Integrator "whitted" is outside the hot-path scope; "path" used']
    assert m.integrator() == ("whitted", 64, True)


def test_path_scenes_warn_as_before(hprt, tmp_path):
    assert _parse(hprt, tmp_path, "p0", "").warnings() == []
    m = _parse(hprt, tmp_path, "p1", 'Integrator "path" "integer maxdepth" [3]')
    assert m.warnings() == [] and m.integrator() == ("path", 64, True) and m.options.max_depth == 3
    # an ambient-occlusion parameter is nothing the path integrator reads
    assert _parse(hprt, tmp_path, "p2", 'Integrator "path" "integer nsamples" [4]').warnings() == ['Parameter "integer nsamples" of Integrator not used']


def test_baked_bytes_do_not_depend_on_the_integrator(hprt, tmp_path):
    a = _parse(hprt, tmp_path, "a", 'Integrator "ambientocclusion" "integer nsamples" [9] "bool cossample" ["false"]')
    b = _parse(hprt, tmp_path, "b", 'Integrator "path"')
    a.save(str(tmp_path / "a.hprt")); b.save(str(tmp_path / "b.hprt"))
    assert (tmp_path / "a.hprt").read_bytes() == (tmp_path / "b.hprt").read_bytes()
    assert hprt.Model.load(str(tmp_path / "a.hprt")).integrator() == ("path", 64, True)      # host side only, not baked


# ---- the restatement against the oracle's sampler ----
def test_array_samples_are_the_oracles_dimensions_5_and_6(hprt, orc, tmp_path):
    n, spp = 5, 3
    m, s = _restated(hprt, tmp_path, "crop", xres=40, yres=30, spp=spp, film='"float cropwindow" [0.3 0.8 0.2 0.9]')
    (cx0, cy0, cx1, cy1), sb = s.bounds()
    assert (cx0, cy0) == (12, 6) and sb[:2] == [12, 6]      # a non-zero sample-bounds origin
    for px, py in [(12, 6), (19, 11), (31, 26)]:
        want_idx = np.array([orc.halton(sb, px, py, j, 5, 2)[0] for j in range(n * spp)], np.uint64)      # GetIndexForSample(s * n + i)
        want = np.stack([orc.halton_dims(sb, want_idx, np.full(n * spp, 5, np.int32)), orc.halton_dims(sb, want_idx, np.full(n * spp, 6, np.int32))], 1)
        u, cam = s.pixel_samples(px, py, n, spp)             # what StartPixel fills, and the camera sample of every pixel sample
        assert np.array_equal(u.view(np.uint32), want.view(np.uint32))
        for k in range(spp):
            # the camera sample still reads dimensions 0 to 4 at GetIndexForSample(k): Get2D's skip test at dimension 3 is false
            assert np.array_equal(cam[k].view(np.uint32), orc.halton(sb, px, py, k, 0, 5)[1].view(np.uint32))
            _, _, _, idx, uk = s.rays(px, py, k, n, True)   # a sample taken on its own
            assert np.array_equal(idx, want_idx[k * n:(k + 1) * n])
            assert np.array_equal(uk.view(np.uint32), want[k * n:(k + 1) * n].view(np.uint32))
    assert len(set(int(v) for v in want_idx)) == n * spp


# ---- the restatement against geometry ----
def test_inside_a_closed_box_the_film_is_zero(hprt, tmp_path):
    m, s = _restated(hprt, tmp_path, "box", body=BOX, spp=2)
    for cos in (True, False):
        film, c = s.render(8, cos)
        assert (film[..., :3] == 0).all() and (film[..., 3] >= 2).all()      # (a sample on a pixel border also lands in the neighbour)
        assert c["camera_rays"] == c["rays"] == 512 and c["shadow_rays"] == 512 * 8      # every camera ray hit a wall


@pytest.mark.parametrize("n", [1, 3, 64])
def test_a_lone_plane_gives_pi_per_sample_under_cosine_sampling(hprt, tmp_path, n):
    """Nothing occludes, and a cosine-distributed direction has Dot(wi, n) / pdf = pi whatever the direction: each term is pi / n up to
    a few roundings (|wi.z| * InvPi, the product with n, the quotient; the frame is the world axes, so Dot(wi, n) is wi.z itself), and
    the sum of n of them adds one rounding each: n * 2^-22 relative covers it."""
    m, s = _restated(hprt, tmp_path, "plane", spp=4)
    px, py = np.meshgrid(np.arange(16), np.arange(16))
    px, py = np.tile(px.ravel(), 4), np.tile(py.ravel(), 4)
    sample = np.repeat(np.arange(4), 256)
    L = s.sample(px, py, sample, n, True).astype(np.float64)
    assert (L[:, 0] == L[:, 1]).all() and (L[:, 0] == L[:, 2]).all()
    rel = np.abs(L[:, 0] - np.pi) / np.pi
    print("n = %d: worst relative distance from pi %.3g (bound %.3g)" % (n, rel.max(), n * 2.0 ** -22))
    assert rel.max() <= n * 2.0 ** -22


def test_a_lone_plane_gives_pi_on_average_under_uniform_sampling(hprt, tmp_path):
    """Dot(wi, n) / (1 / 2 pi) has mean pi and standard deviation 2 pi / sqrt 12 over the hemisphere: the mean of 256 pixels x 4,096
    rays is within 2 % of pi by a wide margin even for a poor sequence — a Monte-Carlo bound, not a device tolerance."""
    spp = 4
    n = 4096 // spp
    m, s = _restated(hprt, tmp_path, "plane_u", spp=spp)
    film, c = s.render(n, False)
    assert c["shadow_rays"] == 256 * spp * n
    # (xyz of a grey L: y = L times the weights' sum; the film holds sums over the pixel's samples)
    mean = float((film[..., 1].astype(np.float64) / film[..., 3]).mean())
    print("uniform sampling, n = %d, spp = %d: mean %.6f" % (n, spp, mean))
    assert abs(mean - np.pi) <= 0.02 * np.pi


# ---- refusals: judged before the scene and the device ----
def _refusal(hprt, fn, n_samples, spp, flags=0):
    m_opt = hprt.RenderOptions()
    m_opt.xres = m_opt.yres = 16
    m_opt.spp = spp
    ao = hprt.AoParams(n_samples, 1)
    if fn == "render":
        desc = hprt.RenderDesc()
        desc.opt = m_opt
        desc.tile_stride, desc.flags = 1, flags
        rc = hprt.lib.hprt_render_ao(None, C.byref(desc), C.byref(ao), None, None, None)
    else:
        rc = hprt.lib.hprt_sample_ao(None, C.byref(m_opt), C.byref(ao), 0, None, None, None, None)
    return rc, hprt.lib.hprt_last_error().decode()


@pytest.mark.parametrize("fn", ["render", "sample"])
def test_sample_counts_outside_1_to_1024_are_invalid(hprt, fn):
    for n in (0, 1025, -3):
        rc, msg = _refusal(hprt, fn, n, 4)
        assert rc == hprt.E_INVALID and "n_samples must lie in 1..1024" in msg, (n, rc, msg)


@pytest.mark.parametrize("fn", ["render", "sample"])
def test_an_overflowing_array_size_is_unsupported(hprt, fn):
    rc, msg = _refusal(hprt, fn, 1024, 1 << 21)          # 2^31 = INT32_MAX + 1
    assert rc == hprt.E_UNSUPPORTED and "INT32_MAX" in msg, (rc, msg)
    rc, msg = _refusal(hprt, fn, 1023, 1 << 21)          # below it: not refused for that (no scene was passed, or no device is there)
    assert rc in (hprt.E_INVALID, hprt.E_NO_DEVICE) and "INT32_MAX" not in msg, (rc, msg)


def test_flags_other_than_count_work_are_unsupported(hprt):
    for flag in (hprt.RENDER_PIXEL_STATS, hprt.RENDER_COUNT_TRACED, hprt.RENDER_TRACE_ALL, hprt.RENDER_EXPORT_FOREIGN, hprt.RENDER_COUNT_WORK | hprt.RENDER_TRACE_ALL):
        rc, msg = _refusal(hprt, "render", 64, 4, flag)
        assert rc == hprt.E_UNSUPPORTED and "only HPRT_RENDER_COUNT_WORK" in msg, (flag, rc, msg)
    rc, msg = _refusal(hprt, "render", 64, 4, hprt.RENDER_COUNT_WORK)
    assert rc in (hprt.E_INVALID, hprt.E_NO_DEVICE) and "HPRT_RENDER_COUNT_WORK" not in msg


def test_the_entry_points_are_exported(hprt):
    for name in ("hprt_model_integrator", "hprt_render_ao", "hprt_sample_ao"):
        assert name in hprt.EXPORTS
