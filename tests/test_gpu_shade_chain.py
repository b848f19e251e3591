"""k_shade's first round of requests (bin entries that carry the hit's primitive word, shape flags and material read from a triangle's
tag, the constant pick of a scene's only light, hit.b requested with the other streams): only the time and the address of loads
changed, so every film here must equal the oracle's bit for bit, also with the workspace poisoned.  The scenes put every shape
flag in front of every shading variant, next to the paths that keep the earlier code: several lights, the spatial distribution
with its retry pass, vertices deferred to the generic bin, escaped rays in the generic bin, and material indices past the inline
maximum (HPRT_INLINE_MATERIAL_MAX)."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _patch(nx=8, ny=8, half=0.42, normals=False, uv=False, tangents=False, amp=0.12):
    """a bumpy nx x ny grid over [-half, half]^2: 2 (nx - 1)(ny - 1) triangles, optionally with "normal N", "float uv", "vector S\""""
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
    dzdx = lambda x, y: amp * 5.1 * np.cos(5.1 * x) * np.cos(4.3 * y)
    dzdy = lambda x, y: -amp * 4.3 * np.sin(5.1 * x) * np.sin(4.3 * y)
    if normals:      # (not normalised, and tilted a little off the surface normal: the shading frame differs from the geometric one)
        s += ' "normal N" [' + fmt([[-dzdx(x, y) + .05, -dzdy(x, y), 1.] for y in ys for x in xs]) + "]"
    if uv:
        s += ' "float uv" [' + fmt([[(x + half) / (2 * half), (y + half) / (2 * half)] for y in ys for x in xs]) + "]"
    if tangents:
        s += ' "vector S" [' + fmt([[1., .1, dzdx(x, y)] for y in ys for x in xs]) + "]"
    return s + "\n"


def _scene(body, xres=96, yres=72, spp=4, maxdepth=5, integ=""):
    return """LookAt 0 -6 3.5  0 0 0.1  0 0 1
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
MATERIALS = [MATTE, PLASTIC, SUBSTRATE, OREN]
# the shape flags: none | N | N, UV, S | REVERSE (ReverseOrientation under a mirroring transform: the two cancel) | FLIP, REVERSE, N
MESHES = [("", _patch()), ("", _patch(normals=True)), ("", _patch(normals=True, uv=True, tangents=True)),
          ("Scale 1 -1 1\nReverseOrientation\n", _patch()), ("ReverseOrientation\n", _patch(normals=True))]


def _every_flag_and_material():
    """5 meshes x 4 materials, 98 triangles each, side by side under the camera"""
    body = ""
    for mi, mat in enumerate(MATERIALS):
        for ki, (xf, mesh) in enumerate(MESHES):
            body += "AttributeBegin\n" + mat + "Translate %g %g 0\n" % (0.9 * (ki - 2), 0.9 * (mi - 1.5)) + xf + mesh + "AttributeEnd\n"
    return body


POINT = 'LightSource "point" "point from" [1 -2 4] "color I" [30 30 30]\n'
POINT2 = 'LightSource "point" "point from" [-2 1 3] "color I" [4 9 16]\n'
GEOM = _every_flag_and_material()
FLOOR = MATTE + 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-4 -4 -.4  4 -4 -.4  4 4 -.4  -4 4 -.4]\n'
_INSTANCED = (
    'LightSource "distant" "point from" [1 -1 3] "point to" [0 0 0] "color L" [2 2 1.5]\n' + FLOOR +
    "".join('ObjectBegin "o%d"\n%s%sObjectEnd\n' % (k, m, _patch(normals=True, uv=(k == 1), tangents=(k == 1))) for k, m in enumerate(MATERIALS)) +
    'AttributeBegin\nTranslate -1.2 0.3 0.2\nRotate 30 0 0 1\nScale 2 2 2\nObjectInstance "o0"\nAttributeEnd\n'
    'AttributeBegin\nTranslate 1.1 -0.4 0.1\nRotate -50 0.2 0.1 1\nScale 2.6 1.6 2.2\nObjectInstance "o1"\nAttributeEnd\n'
    'AttributeBegin\nTranslate 0 1.2 0.5\nScale 2 -2 2\nObjectInstance "o2"\nAttributeEnd\n'
    'AttributeBegin\nTranslate 0 -1.1 0.3\nScale 2 2 2\nObjectInstance "o3"\nAttributeEnd\n'
    'AttributeBegin\nTranslate -1.5 -1.2 0.3\nScale 1.5 1.5 1.5\nObjectInstance "o1"\nAttributeEnd\nObjectInstance "o0"\n')
NORMAL_MESHES = "".join("AttributeBegin\n%sTranslate %g %g 0\nScale 2 2 2\n%sAttributeEnd\n" % (m, 1.8 * (k % 2) - .9, 1.8 * (k // 2) - .9, _patch(normals=True))
                        for k, m in enumerate(MATERIALS))

CASES = {
    # C's constant pick together with every flag combination read from the tag, in every variant
    "one_point_light_every_shape_flag": _scene(POINT + GEOM),
    # the unchanged pick beside the new bin entries
    "two_point_lights_uniform": _scene(POINT + POINT2 + GEOM, integ='"string lightsamplestrategy" "uniform"'),
    "two_point_lights_power": _scene(POINT + POINT2 + GEOM, integ='"string lightsamplestrategy" "power"'),
    # the variants compiled with the instance transform
    "one_distant_light_instances_with_normals": _scene(_INSTANCED, xres=40, yres=30),
    # a sphere emitter, open at the top so that the camera sees into it, with the geometry inside it: the specialised variants defer such vertices to the generic bin, with their word
    "deferral_inside_a_sphere_emitter": _scene('AttributeBegin\nMaterial "matte" "color Kd" [0 0 0]\nTranslate .3 -.2 .3\nAreaLightSource "area" "color L" [3 2.8 2.4]\n'
                                               'Shape "sphere" "float radius" [1.6] "float zmax" [.3]\nAttributeEnd\n' + PLASTIC + "Scale 2 2 2\n" + _patch(normals=True) + MATTE +
                                               "Translate 0 0 -.2\n" + _patch(nx=3, ny=3, half=1.5, amp=0.)),
    # three lights, the default (spatial) strategy: rendered again with the voxels filled on demand, whose retry pass reads the word from hit.a
    "three_lights_spatial_retry": _scene(POINT + POINT2 + 'LightSource "distant" "point from" [-1 -1 3] "point to" [0 0 0] "color L" [.5 1 .5]\n' + FLOOR + NORMAL_MESHES),
    # an infinite light: escaped camera rays sit in the generic bin with a negative word and must not index the primitive records
    "escaped_rays_in_the_generic_bin": _scene('LightSource "infinite" "rgb L" [.4 .45 .5]\n' + PLASTIC + _patch(normals=True) + OREN + "Translate 1 0 0\n" + _patch()),
}

_cache = {}


def _load(hprt, orc, tmp_path_factory, name):
    """(model, bvh, the oracle's film): parsed, baked and rendered by the oracle once per scene"""
    if name not in _cache:
        d = tmp_path_factory.mktemp(name)
        p = d / (name + ".pbrt")
        p.write_text(CASES[name])
        model = hprt.Model.parse(str(p))
        assert model.warnings() == [], model.warnings()
        baked = str(d / (name + ".hprt"))
        model.save(baked)
        _, film0, _, _, _ = orc.OracleScene(baked).render(threads=8)
        assert film0[..., :3].max() > 0
        film0.setflags(write=False)
        _cache[name] = (model, hprt.Bvh(model), film0)
    return _cache[name]


def _same(film, film0, what):
    assert film.shape == film0.shape
    bad = np.any(film0.view(np.uint32) != film.view(np.uint32), axis=2)
    assert np.array_equal(film.view(np.uint32), film0.view(np.uint32)), "%s: %d pixels differ, max |d| = %g" % (what, int(bad.sum()), float(np.abs(film0 - film).max()))


def _render_twice(scene, film0, what):
    """the plain render, and the same with garbage in every scratch stream, queue and stack: both the oracle's film"""
    film, st = scene.render()
    _same(film, film0, what)
    scene.debug_poison(0xFF)
    try:
        poisoned, _ = scene.render()
    finally:
        scene.debug_poison(None)
    _same(poisoned, film0, what + " (poisoned)")
    return film, st


def _shade_counts(hprt, scene, on):
    """hprt_debug_shade_counts: (vertices the specialised variants deferred to the generic bin, vertices shaded again by a retry pass) since
    the counting was switched on"""
    fn = hprt.lib.hprt_debug_shade_counts
    fn.restype = C.c_int; fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 2)()
    assert fn(scene._h, int(on), out) == 0
    return int(out[0]), int(out[1])


def _scene_with_env(hprt, model, bvh, key, value):
    old = os.environ.get(key)
    os.environ[key] = value
    try:
        return hprt.Scene(model, bvh)
    finally:
        if old is None:
            del os.environ[key]
        else:
            os.environ[key] = old


@pytest.mark.parametrize("name", sorted(CASES))
def test_film_equals_the_oracle(hprt, orc, tmp_path_factory, name):
    model, bvh, film0 = _load(hprt, orc, tmp_path_factory, name)
    if name == "one_point_light_every_shape_flag":
        c = model.counts()
        assert c["materials"] >= 4 and c["lights"] == 1, c
    scene = hprt.Scene(model, bvh)
    _shade_counts(hprt, scene, True)
    film, st = _render_twice(scene, film0, name)
    deferred, retried = _shade_counts(hprt, scene, False)
    # the rare paths are really taken where a case is about them (every voxel has its row here: nothing waits for a retry)
    if name == "deferral_inside_a_sphere_emitter":
        assert deferred > 0
    assert retried == 0
    if name == "escaped_rays_in_the_generic_bin":
        # the corners see no geometry: their radiance comes from escaped camera rays alone, which only the generic variant's bin-2 entries add
        assert min(film[0, 0, :3].max(), film[-1, -1, :3].max(), film[0, -1, :3].max()) > 0
    if name == "three_lights_spatial_retry":
        lazy = _scene_with_env(hprt, model, bvh, "HPRT_VOXEL_DENSE_MAX_MB", "0")      # voxel rows on demand + the retry pass
        _shade_counts(hprt, lazy, True)
        _, st_lazy = _render_twice(lazy, film0, name + ", on-demand voxels")
        assert (st_lazy["rays"], st_lazy["shadow_rays"]) == (st["rays"], st["shadow_rays"])
        assert _shade_counts(hprt, lazy, False)[1] > 0


def test_inline_fallback(hprt, orc, tmp_path_factory):
    """material indices 2 and 3 past the inline maximum: their triangles' flags and material come from shapes[] again, the film stays"""
    name = "one_point_light_every_shape_flag"
    model, bvh, film0 = _load(hprt, orc, tmp_path_factory, name)
    plain, _ = hprt.Scene(model, bvh).render()
    scene = _scene_with_env(hprt, model, bvh, "HPRT_INLINE_MATERIAL_MAX", "1")
    film, _ = _render_twice(scene, film0, name + ", HPRT_INLINE_MATERIAL_MAX=1")
    assert np.array_equal(film.view(np.uint32), plain.view(np.uint32))
