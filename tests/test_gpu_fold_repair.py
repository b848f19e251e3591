"""The repair of a blocked speculated light sample, folded into the next bounce: a speculated vertex whose path goes on marks its
outgoing segment (RAY_FOLD_MARK), and whoever reads the vertex's radiance next — k_shade of the next bounce, or k_bin for a path that
ends at the bin — takes the record's dark value instead where the shadow ray turned out blocked.  k_repair only runs over the
speculated vertices at which a path ends.  The choice between two stored values involves no arithmetic, so every film here must be
identical, as uint32, to the render with hprt_debug_fold_repair(0) (every shadow ray through k_repair, nothing marked) and to the
render with hprt_debug_speculate_light(0) (every pending term through k_resolve).  A counting render (which keeps the unfolded flow)
shows that the scene has vertices of both outcomes to get wrong."""
import ctypes as C
import os

import numpy as np
import pytest

from test_gpu_speculated_light import (DISTANT, FLOOR, GLASS, INSTANCED, MATTE, OCCLUDERS, PLASTIC, POINT, POINT2, SPHERE_LIGHT,
                                       _counting, _counts, _old_path, _patch, _same, _scene)

pytestmark = pytest.mark.gpu


def _quad(p):
    return 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [%s]\n' % " ".join("%g" % v for v in p)


# a closed room around the camera (0 -6 3.5) and the light (1 -2 4): matte floor and ceiling, plastic walls, and one bumpy matte patch
# floating over the floor.  Nothing escapes, so below the depth limit every path goes on.
ROOM = (MATTE + _quad([-8, -8, -.4, 8, -8, -.4, 8, 8, -.4, -8, 8, -.4]) + _quad([-8, -8, 7, 8, -8, 7, 8, 8, 7, -8, 8, 7]) +
        PLASTIC + _quad([-8, -8, -.4, -8, 8, -.4, -8, 8, 7, -8, -8, 7]) + _quad([8, -8, -.4, 8, 8, -.4, 8, 8, 7, 8, -8, 7]) +
        _quad([-8, -8, -.4, 8, -8, -.4, 8, -8, 7, -8, -8, 7]) + _quad([-8, 8, -.4, 8, 8, -.4, 8, 8, 7, -8, 8, 7]) +
        "AttributeBegin\n" + MATTE + "Translate .2 -.3 .6\nScale 3 3 2\n" + _patch() + "AttributeEnd\n")
# a wall between the camera and the light: the face the camera sees looks away from the light (no shadow ray from it: f is black), and the
# floor behind it lies in its shadow
AWAY = MATTE + _quad([-3, -3, -.4, .5, -3, -.4, .5, -3, 2.2, -3, -3, 2.2])
# a sphere emitter open at the top with geometry inside it (the specialised variants defer those vertices to the generic bin), and a point
# light whose samples the same vertices speculate
DEFER = ('AttributeBegin\nMaterial "matte" "color Kd" [0 0 0]\nTranslate .3 -.2 .3\nAreaLightSource "area" "color L" [3 2.8 2.4]\n'
         'Shape "sphere" "float radius" [1.6] "float zmax" [.3]\nAttributeEnd\n' + POINT +
         "AttributeBegin\n" + PLASTIC + "Translate 0 0 .5\nScale 2 2 2\n" + _patch(normals=True) + "AttributeEnd\n" +
         MATTE + "Translate 0 0 -.2\n" + _patch(nx=3, ny=3, half=2.5, amp=0.))

S = dict(xres=64, yres=64)
CASES = {
    # (a) blocked and unblocked vertices on paths that go on, at every bounce
    "a_closed_room": (_scene(POINT + ROOM, spp=4, maxdepth=3, **S), {}),
    # (b) every vertex ends its path: nothing is marked, everything goes through the end queue
    "b_closed_room_maxdepth1": (_scene(POINT + ROOM, spp=4, maxdepth=1, **S), {}),
    # (c) paths escape and end in k_bin right after a blocked vertex
    "c_open": (_scene(POINT + OCCLUDERS, spp=4, **S), {}),
    # (d) etaScale != 1 must survive the choice in L.w
    "d_glass": (_scene(POINT + OCCLUDERS + GLASS, spp=4, maxdepth=8, integ='"float rrthreshold" [1]', **S), {}),
    # (e) vertices without a shadow ray at slots whose occlusion byte an earlier bounce, batch or render set
    "e_facing_away": (_scene(POINT + OCCLUDERS + AWAY, spp=4, **S), {"twice": True}),
    # (f) three batches of unequal size (3 + 3 + 2): plane parity and stale bytes across batches
    "f_three_batches": (_scene(POINT + ROOM, spp=8, maxdepth=4, **S), {"spp_chunk": 3}),
    # (g) speculated vertices beside MIS vertices: k_resolve and the fold in one bounce
    "g_sphere_emitter": (_scene(SPHERE_LIGHT + OCCLUDERS, spp=4, **S), {}),
    # (h) the spatial light distribution with on-demand voxels (the retry pass), and vertices deferred to the generic bin
    "h_spatial_on_demand": (_scene(POINT + POINT2 + DISTANT + OCCLUDERS, spp=4, **S), {"lazy_voxels": True, "retried": True}),
    "h_deferred_to_generic": (_scene(DEFER, spp=4, **S), {"deferred": True}),
    # (i) the variants compiled with the instance transform
    "i_instances": (_scene(INSTANCED, xres=40, yres=30), {}),
}


class _unfolded:
    """hprt_debug_fold_repair(0) for the renders inside"""
    def __init__(self, hprt):
        self.fn = hprt.lib.hprt_debug_fold_repair
        self.fn.restype = C.c_int; self.fn.argtypes = [C.c_int]

    def __enter__(self):
        self.was = self.fn(0)

    def __exit__(self, *a):
        self.fn(-1 if self.was else 0)      # (-1: back to the environment's setting)


def _shade_counts(hprt, scene):
    """hprt_debug_shade_counts: (deferred, retried) so far; counting stays as it is"""
    fn = hprt.lib.hprt_debug_shade_counts
    fn.restype = C.c_int; fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 2)()
    assert fn(scene._h, 1, out) == 0
    return int(out[0]), int(out[1])


def _make_scene(hprt, model, lazy_voxels):
    if not lazy_voxels:
        return hprt.Scene(model, hprt.Bvh(model))
    old = os.environ.get("HPRT_VOXEL_DENSE_MAX_MB")
    os.environ["HPRT_VOXEL_DENSE_MAX_MB"] = "0"      # voxel rows on demand + the retry pass
    try:
        return hprt.Scene(model, hprt.Bvh(model))
    finally:
        if old is None:
            del os.environ["HPRT_VOXEL_DENSE_MAX_MB"]
        else:
            os.environ["HPRT_VOXEL_DENSE_MAX_MB"] = old


@pytest.mark.parametrize("name", sorted(CASES))
def test_folded_unfolded_and_resolved_films_are_identical(hprt, tmp_path, name):
    text, how = CASES[name]
    p = tmp_path / (name + ".pbrt")
    p.write_text(text)
    model = hprt.Model.parse(str(p))
    assert model.warnings() == [], model.warnings()
    lazy = how.get("lazy_voxels", False)
    first = _make_scene(hprt, model, lazy)
    # (voxel rows filled on demand stay filled: only a scene's first render runs the retry pass, so those cases render on fresh scenes)
    scene = (lambda: _make_scene(hprt, model, True)) if lazy else (lambda: first)
    kw = {"spp_chunk": how.get("spp_chunk", 0)}
    folded, st = first.render(**kw)
    assert np.isfinite(folded).all() and folded[..., :3].max() > 0
    if how.get("twice"):      # the workspace now holds the first render's occlusion bytes
        again, _ = first.render(**kw)
        _same(again, folded, name + " (second render)")
    for byte in (0xFF, 0x01):      # every stale occlusion byte reads "blocked"; 0xFF also sets every bit of a stale segment word
        sc = scene()
        sc.debug_poison(byte)
        try:
            poisoned, _ = sc.render(**kw)
            if how.get("twice"):
                poisoned2, _ = sc.render(**kw)
                _same(poisoned2, folded, name + " (poisoned %#x, second render)" % byte)
        finally:
            sc.debug_poison(None)
        _same(poisoned, folded, name + " (poisoned %#x)" % byte)
    with _unfolded(hprt):
        unfolded, st_u = scene().render(**kw)
    _same(unfolded, folded, name + " (fold off)")
    with _old_path(hprt):
        resolved, st_r = scene().render(**kw)
    _same(resolved, folded, name + " (no speculation)")
    assert (st_u["rays"], st_u["shadow_rays"]) == (st["rays"], st["shadow_rays"]) == (st_r["rays"], st_r["shadow_rays"])
    # what the scene exercises, from a counting render (unfolded flow): blocked and unblocked speculated vertices
    sc = scene()
    _counting(hprt, sc, True)
    counted, _ = sc.render(**kw)
    speculated, repaired, full = _counts(hprt, sc)
    deferred, retried = _shade_counts(hprt, sc)
    _counting(hprt, sc, False)
    _same(counted, folded, name + " (counting render)")
    print("%s: speculated %d, repaired %d, full %d, deferred %d, retried %d" % (name, speculated, repaired, full, deferred, retried))
    assert 0 < repaired < speculated
    if name == "g_sphere_emitter":
        assert full > 0
    if how.get("deferred"):
        assert deferred > 0
    if how.get("retried"):
        assert retried > 0
