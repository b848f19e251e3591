"""Speculated light samples: k_shade adds the light sample of a vertex that has a shadow ray and no MIS ray at once and leaves
the value without it in a record; k_repair puts that value back where the shadow ray was blocked.  Vertices with an MIS ray keep
the pending streams and k_resolve.  Both ways form the same sums with the same operations, so every film here must equal the
oracle's bit for bit, and the render with the switch on the old path (hprt_debug_speculate_light(0): every pending term through
k_resolve) as well — some with the workspace poisoned.  hprt_debug_speculated_counts proves that each branch ran."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _patch(nx=8, ny=8, half=0.42, normals=False, amp=0.12):
    """a bumpy nx x ny grid over [-half, half]^2: 2 (nx - 1)(ny - 1) triangles, optionally with "normal N\""""
    xs = np.linspace(-half, half, nx); ys = np.linspace(-half, half, ny)
    z = lambda x, y: amp * np.sin(5.1 * x) * np.cos(4.3 * y)
    P = np.array([[x, y, z(x, y)] for y in ys for x in xs], np.float32)
    idx = []
    for j in range(ny - 1):
        for i in range(nx - 1):
            a = j * nx + i
            idx += [a, a + 1, a + nx + 1, a, a + nx + 1, a + nx]
    fmt = lambda a: " ".join("%r" % float(v) for v in np.asarray(a, np.float32).ravel())
    s = 'Shape "trianglemesh" "integer indices" [' + " ".join(map(str, idx)) + '] "point P" [' + fmt(P) + "]"
    if normals:
        dzdx = lambda x, y: amp * 5.1 * np.cos(5.1 * x) * np.cos(4.3 * y)
        dzdy = lambda x, y: -amp * 4.3 * np.sin(5.1 * x) * np.sin(4.3 * y)
        s += ' "normal N" [' + fmt([[-dzdx(x, y) + .05, -dzdy(x, y), 1.] for y in ys for x in xs]) + "]"
    return s + "\n"


def _scene(body, xres=96, yres=72, spp=4, maxdepth=5, integ=""):
    return """LookAt 0 -6 3.5  0 0 0.3  0 0 1
Camera "perspective" "float fov" [40]
Film "image" "integer xresolution" [%d] "integer yresolution" [%d]
Sampler "halton" "integer pixelsamples" [%d]
Integrator "path" "integer maxdepth" [%d] %s
WorldBegin
%s
WorldEnd
""" % (xres, yres, spp, maxdepth, integ, body)


MATTE = 'Material "matte" "color Kd" [.6 .5 .3]\n'
PLASTIC = 'Material "plastic" "color Kd" [.2 .3 .5] "color Ks" [.6 .6 .6] "float roughness" [.08]\n'
SUBSTRATE = 'Material "substrate" "color Kd" [.5 .3 .2] "color Ks" [.04 .04 .04] "float uroughness" [.15] "float vroughness" [.05] "bool remaproughness" "false"\n'
OREN = 'Material "matte" "color Kd" [.3 .6 .4] "float sigma" [35]\n'      # OrenNayar: shaded by the generic variant
POINT = 'LightSource "point" "point from" [1 -2 4] "color I" [30 30 30]\n'
POINT2 = 'LightSource "point" "point from" [-2 1 3] "color I" [4 9 16]\n'
DISTANT = 'LightSource "distant" "point from" [-1 -1 3] "point to" [0 0 0] "color L" [.5 1 .5]\n'
SPHERE_LIGHT = 'AttributeBegin\nMaterial "matte" "color Kd" [0 0 0]\nTranslate 1.5 -1 3\nAreaLightSource "area" "color L" [40 38 30]\nShape "sphere" "float radius" [0.35]\nAttributeEnd\n'
FLOOR = MATTE + 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-4 -4 -.4  4 -4 -.4  4 4 -.4  -4 4 -.4]\n'
# a matte floor under two matte and two plastic patches that float above it: the patches shadow the floor and one another
OCCLUDERS = FLOOR + "".join("AttributeBegin\n%sTranslate %g %g %g\nScale 2 2 2\n%sAttributeEnd\n" % (m, 1.8 * (k % 2) - .9, 1.8 * (k // 2) - .9, .25 * k, _patch(normals=(k > 1)))
                            for k, m in enumerate([MATTE, PLASTIC, PLASTIC, MATTE]))
GLASS = ('AttributeBegin\nMaterial "glass"\nTranslate -1.0 -.2 .55\nShape "sphere" "float radius" [.5]\nAttributeEnd\n'
         # one open sheet between the camera and the floor: a path that crosses it once keeps etaScale = 1 / eta^2 (or eta^2) for good
         'AttributeBegin\nMaterial "glass" "float index" [1.33]\n'
         'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-.2 -2.2 .1  2.2 -2.2 .1  2.2 -1.6 1.6  -.2 -1.6 1.6]\nAttributeEnd\n')
INSTANCED = ('LightSource "distant" "point from" [1 -1 3] "point to" [0 0 0] "color L" [2 2 1.5]\n' + FLOOR +
             "".join('ObjectBegin "o%d"\n%s%sObjectEnd\n' % (k, m, _patch(normals=True)) for k, m in enumerate([MATTE, PLASTIC, SUBSTRATE, OREN])) +
             'AttributeBegin\nTranslate -1.2 0.3 0.2\nRotate 30 0 0 1\nScale 2 2 2\nObjectInstance "o0"\nAttributeEnd\n'
             'AttributeBegin\nTranslate 1.1 -0.4 0.1\nRotate -50 0.2 0.1 1\nScale 2.6 1.6 2.2\nObjectInstance "o1"\nAttributeEnd\n'
             'AttributeBegin\nTranslate 0 1.2 0.5\nScale 2 -2 2\nObjectInstance "o2"\nAttributeEnd\n'
             'AttributeBegin\nTranslate 0 -1.1 0.3\nScale 2 2 2\nObjectInstance "o3"\nAttributeEnd\nObjectInstance "o0"\n')

CASES = {
    # (a) both outcomes of a speculated vertex, on paths that go on and on paths that end there (maxdepth 1: every vertex is a last one)
    "point_light_occluders": _scene(POINT + OCCLUDERS),
    "point_light_occluders_maxdepth1": _scene(POINT + OCCLUDERS, maxdepth=1),
    # (b) a sphere emitter: vertices with a shadow ray only (speculated) beside shadow + MIS and MIS only (full)
    "sphere_light": _scene(SPHERE_LIGHT + OCCLUDERS),
    # (c) etaScale != 1 in out.L.w of vertices behind the glass, shadowed by the patches and the glass itself: the repair leaves it
    "point_light_through_glass": _scene(POINT + OCCLUDERS + GLASS, maxdepth=10, integ='"float rrthreshold" [1]'),
    # (d) the spatial distribution: the pick pdf is the vertex's own; rendered again with the voxels filled on demand (the retry pass speculates too)
    "three_lights_spatial": _scene(POINT + POINT2 + DISTANT + OCCLUDERS),
    # (e) alpha 0 along one axis: beta turns NaN, and the dark value must be NaN where the reference's guard zeroes the sample
    "rough_glass_degenerate_alpha": _scene(
        'LightSource "point" "point from" [1 -2 4] "color I" [20 18 15]\n' + SPHERE_LIGHT + OCCLUDERS +
        'AttributeBegin\nMaterial "glass" "float index" [1.31] "float uroughness" [0] "float vroughness" [.4] "bool remaproughness" "false"\n'
        'Translate -1.0 -.2 .55\nShape "sphere" "float radius" [.5]\nAttributeEnd\n'
        'AttributeBegin\nMaterial "glass" "color Kt" [0 0 0] "float uroughness" [.05] "float vroughness" [0] "bool remaproughness" "false"\n'
        'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [.3 -1.4 .05  1.7 -1.4 .05  1.7 -.6 .6  .3 -.6 .6]\nAttributeEnd\n',
        integ='"string lightsamplestrategy" "power"', maxdepth=6),
    # (f) the variants compiled with the instance transform
    "distant_light_instances": _scene(INSTANCED, xres=40, yres=30),
}
POISONED = {"point_light_occluders", "point_light_occluders_maxdepth1", "sphere_light", "three_lights_spatial"}

_cache = {}


def _load(hprt, orc, tmp_path_factory, name):
    """(model, bvh, the oracle's film, the oracle): parsed, baked and rendered by the oracle once per scene"""
    if name not in _cache:
        d = tmp_path_factory.mktemp(name)
        p = d / (name + ".pbrt")
        p.write_text(CASES[name])
        model = hprt.Model.parse(str(p))
        assert model.warnings() == [], model.warnings()
        baked = str(d / (name + ".hprt"))
        model.save(baked)
        oracle = orc.OracleScene(baked)
        _, film0, _, _, _ = oracle.render(threads=8)
        assert film0[..., :3].max() > 0
        film0.setflags(write=False)
        _cache[name] = (model, hprt.Bvh(model), film0, oracle)
    return _cache[name]


def _same(film, film0, what):
    assert film.shape == film0.shape
    bad = np.any(film0.view(np.uint32) != film.view(np.uint32), axis=2)
    assert np.array_equal(film.view(np.uint32), film0.view(np.uint32)), "%s: %d pixels differ, max |d| = %g" % (what, int(bad.sum()), float(np.abs(film0 - film).max()))


def _counting(hprt, scene, on):
    fn = hprt.lib.hprt_debug_shade_counts
    fn.restype = C.c_int; fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 2)()
    assert fn(scene._h, int(on), out) == 0
    return int(out[1])      # vertices shaded again by a retry pass


def _counts(hprt, scene):
    """hprt_debug_speculated_counts: (speculated, repaired, full) vertices since the counting was switched on"""
    fn = hprt.lib.hprt_debug_speculated_counts
    fn.restype = C.c_int; fn.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 3)()
    assert fn(scene._h, out) == 0
    return int(out[0]), int(out[1]), int(out[2])


class _old_path:
    """hprt_debug_speculate_light(0) for the renders inside"""
    def __init__(self, hprt):
        self.fn = hprt.lib.hprt_debug_speculate_light
        self.fn.restype = C.c_int; self.fn.argtypes = [C.c_int]

    def __enter__(self):
        self.was = self.fn(0)

    def __exit__(self, *a):
        self.fn(-1 if self.was else 0)      # (-1: back to the environment's setting)


def _check(hprt, scene, film0, name, poisoned):
    """the default render, counted; the same poisoned; the old path (counted too): all the oracle's film.  Returns both count triples."""
    _counting(hprt, scene, True)
    film, st = scene.render()
    new = _counts(hprt, scene)
    retried = _counting(hprt, scene, False)
    _same(film, film0, name)
    if poisoned:
        scene.debug_poison(0xFF)
        try:
            again, _ = scene.render()
        finally:
            scene.debug_poison(None)
        _same(again, film0, name + " (poisoned)")
    with _old_path(hprt):
        _counting(hprt, scene, True)
        old, st_old = scene.render()
        oldc = _counts(hprt, scene)
        _counting(hprt, scene, False)
    _same(old, film0, name + " (old path)")
    assert np.array_equal(old.view(np.uint32), film.view(np.uint32))
    assert (st_old["rays"], st_old["shadow_rays"]) == (st["rays"], st["shadow_rays"])
    # the old path speculates nothing, and every vertex with a pending term is one or the other
    assert oldc[0] == 0 and oldc[1] == 0 and oldc[2] == new[0] + new[2], (new, oldc)
    assert new[1] <= new[0] <= st["shadow_rays"]
    return new, oldc, retried


@pytest.mark.parametrize("name", sorted(CASES))
def test_film_equals_the_oracle_and_the_old_path(hprt, orc, tmp_path_factory, name):
    model, bvh, film0, _ = _load(hprt, orc, tmp_path_factory, name)
    scene = hprt.Scene(model, bvh)
    (speculated, repaired, full), _, retried = _check(hprt, scene, film0, name, name in POISONED)
    print("%s: speculated %d, repaired %d (%.3f), full %d" % (name, speculated, repaired, repaired / max(speculated, 1), full))
    assert retried == 0
    assert repaired > 0 and speculated > repaired      # both outcomes
    if name in ("point_light_occluders", "point_light_occluders_maxdepth1", "point_light_through_glass", "distant_light_instances", "three_lights_spatial"):
        assert full == 0      # point and distant lights have no BSDF-sampled term
    if name in ("sphere_light", "rough_glass_degenerate_alpha"):
        assert full > 0
    if name == "rough_glass_degenerate_alpha":
        assert np.isfinite(film0).all()
    if name == "three_lights_spatial":
        old = os.environ.get("HPRT_VOXEL_DENSE_MAX_MB")
        os.environ["HPRT_VOXEL_DENSE_MAX_MB"] = "0"      # voxel rows on demand + the retry pass
        try:
            lazy = hprt.Scene(model, bvh)
        finally:
            if old is None:
                del os.environ["HPRT_VOXEL_DENSE_MAX_MB"]
            else:
                os.environ["HPRT_VOXEL_DENSE_MAX_MB"] = old
        lazy_counts, _, lazy_retried = _check(hprt, lazy, film0, name + ", on-demand voxels", True)
        assert lazy_retried > 0 and lazy_counts == (speculated, repaired, full)


def test_pixel_statistics_keep_the_old_path(hprt, orc, tmp_path_factory):
    """(g) a per-pixel-statistics render reads pendBeta.w of every shadow ray as a plain path id: nothing is speculated there, and
    its matrices and film are the oracle's"""
    name = "point_light_occluders"
    model, bvh, film0, oracle = _load(hprt, orc, tmp_path_factory, name)
    ref = oracle.pixel_stats()
    scene = hprt.Scene(model, bvh)
    _counting(hprt, scene, True)
    film, st = scene.render(pixel_stats=True)
    speculated, repaired, full = _counts(hprt, scene)
    _counting(hprt, scene, False)
    assert np.array_equal(scene.pixel_stats(), ref)
    _same(film, film0, name + " (pixel statistics)")
    assert speculated == 0 and repaired == 0 and full > 0
