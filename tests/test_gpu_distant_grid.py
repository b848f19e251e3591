"""k_distant_grid (csrc/device/distant_grid.hip) on the GPU: the any-hit answers of distant-light shadow rays from the
light-aligned candidate grid are the walk's and the oracle's, byte for byte, and films rendered through it are the films rendered
through the walk, bit for bit.

Scenes and rays: tests/distant_grid_cases.py — every ray formed in float32 as a render forms it (T = p + w * 2 worldRadius, o =
OffsetRayOrigin(p, pErr, n, T - p), d = T - o, tMax = 1 - ShadowEpsilon): origins on triangles, origins whose projection lies on
cell and sixteenth boundaries (exactly, under the axis-aligned lights), at the key seam (a triangle's top height +- 0, 1, 2, 8 ulps),
above and below everything, along edges and through vertices, at and past the rectangle's rim, and with tMax > 1.
tests/test_distant_grid_host.py holds that the oracle reports between 5 % and 95 % of every family occluded.  R = 8 makes every list
long, 64 and the default exercise the margins.  Scenes are created with HPRT_SHADOW_GRID=1 where the lists may be long."""
import os
import subprocess
import sys

import numpy as np
import pytest

import distant_grid_cases as dgc
import shadow_grid_cases as sgc
from shadow_grid_cases import grid_scene as _scene
from conftest import ROOT

pytestmark = pytest.mark.gpu

F = np.float32
CUTS = (0, 1, 2, 3, 4, -1)      # the entry in front of which the key cut falls; -1: behind the list's last key


def _rays7(o, d, tm):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.concatenate([o.T, d.T, tm[None, :]]).astype(F))).to("cuda:0")


def _walk(scene, rays7, n):
    import torch
    occ = torch.full((n,), 7, dtype=torch.uint8, device="cuda:0")
    scene.occluded_device(n, rays7.data_ptr(), occ.data_ptr())
    torch.cuda.synchronize()
    return occ.cpu().numpy()


def _grid(scene, rays7, n):
    import torch
    occ = torch.full((n,), 7, dtype=torch.uint8, device="cuda:0")
    scene.distant_grid_occluded_device(n, rays7.data_ptr(), occ.data_ptr())
    return occ.cpu().numpy()


@pytest.fixture(scope="module")
def cases(hprt, orc, tmp_path_factory):
    """per scene: the model, the rays of every family, and the answers of the walk and of the oracle — computed once, shared by the R's"""
    tmp = str(tmp_path_factory.mktemp("dg"))
    out = {}
    for name in dgc.NAMES:
        model, path, p9, w = dgc.bake(hprt, name, tmp)
        rays = dgc.family_rays(p9, w, hprt.distant_grid_build(p9, w, 64))
        family = np.concatenate([np.full(r[0].shape[0], k) for k, r in enumerate(rays.values())])
        o, d, tm = (np.concatenate([r[k] for r in rays.values()]) for k in range(3))
        assert 100000 < o.shape[0] <= 140000
        walk_scene = _scene(hprt, model, grid="0")
        assert not walk_scene.distant_grid_info()["eligible"] and not walk_scene.shadow_grid_info()["eligible"]
        rays7 = _rays7(o, d, tm)
        out[name] = {"model": model, "path": path, "p9": p9, "w": w, "o": o, "d": d, "tm": tm, "family": family, "families": list(rays),
                     "rays7": rays7, "walk": _walk(walk_scene, rays7, o.shape[0]), "oracle": orc.OracleScene(path).occluded(o, d, tm)[0]}
    return out


@pytest.mark.parametrize("res", [8, 64, None])
@pytest.mark.parametrize("name", dgc.NAMES)
def test_grid_answers_are_the_walks_and_the_oracles(hprt, cases, name, res):
    c = cases[name]
    assert np.array_equal(c["walk"], np.asarray(c["oracle"], np.uint8))
    for k, fam in enumerate(c["families"]):
        share = c["walk"][c["family"] == k].mean()
        assert 0.05 <= share <= 0.95, (name, fam, share)
    scene = _scene(hprt, c["model"], res)
    info = scene.distant_grid_info()
    assert info["eligible"] and np.array_equal(info["w"], c["w"]) and info["R"] == (hprt.DG_DEFAULT_RES if res is None else res), info
    assert info["near"] == 0 and not scene.shadow_grid_info()["eligible"]
    g = hprt.distant_grid_build(c["p9"], c["w"], info["R"])
    assert np.array_equal(info["U"], g["U"]) and np.array_equal(info["V"], g["V"]) and info["entries"] == g["prim"].size
    got = _grid(scene, c["rays7"], c["o"].shape[0])
    bad = np.nonzero(got != c["walk"])[0]
    assert bad.size == 0, (name, res, bad.size, bad[:8], got[bad[:8]], c["family"][bad[:8]], c["o"][bad[:4]], c["d"][bad[:4]])
    # under the axis-aligned lights the boundary family did put projections exactly on column boundaries, as the device computes them
    if name in ("soup_axis", "axis", "dodecahedron"):
        o = c["o"][c["family"] == c["families"].index("boundary")]
        exact = np.zeros(o.shape[0], bool)
        for a, x0, s in ((g["U"], g["u0"], g["scale_u"]), (g["V"], g["v0"], g["scale_v"])):
            pu = ((o[:, 0] * a[0]).astype(F) + (o[:, 1] * a[1]).astype(F) + (o[:, 2] * a[2]).astype(F)).astype(F)
            x = ((pu - x0).astype(F) * s).astype(F)
            exact |= (x == np.floor(x)) & (x > 0) & (x < 16 * info["R"])
        assert exact.sum() > 1000, (name, res, int(exact.sum()))


def _seam_texts():
    P, idx = sgc.soup(150, 21, centre_lo=-2.5, centre_hi=2.5, size=0.5)
    twice = np.concatenate([idx, idx[:, [1, 2, 0]]])      # every triangle twice: equal bounds and centroids, so a leaf holds both
    nanP = np.array([[0, 0, 0], [1, 0, 0], [0, 1, np.nan]], np.float32)
    return {"soup": dgc.scenes()["soup"],
            "pairs": dgc.scene_text(dgc.GENERIC, [(P, twice), sgc.floor()]),
            "near": dgc.scene_text(dgc.GENERIC, [(nanP, np.arange(3).reshape(1, 3)), sgc.soup(300, 2), sgc.floor()])}


def _aimed(im, g, rng, cuts):
    """origins inside cells whose key cut falls at the entries of `cuts`, and the cut each was aimed at"""
    keys = (im["key_word"] & np.uint32(0xffff0000)).view(F).astype(np.float64)
    cs, count = im["cell_start"], im["count"]
    R = g["R"]
    U, V, W = (g[k].astype(np.float64) for k in "UVW")
    out, aim = [], []
    for cut in cuts:
        cells = np.nonzero(count >= max(1, cut + 1))[0]
        if cut > 0:
            cells = cells[keys[cs[cells] + cut - 1] < keys[cs[cells] + cut]]
        elif cut == 0:
            cells = cells[keys[cs[cells]] > 0]
        if cells.size == 0:      # (R = 1: the one list need not change its 16-bit key at every one of its first entries)
            assert R == 1, cut
            continue
        cells = rng.permutation(np.repeat(cells, -(-400 // cells.size)))[:400]
        first = cs[cells]
        if cut == 0:
            lim = keys[first] * 0.9
        elif cut < 0:
            lim = keys[first + count[cells] - 1] * 1.1 + 1e-3
        else:
            lim = 0.5 * (keys[first + cut - 1] + keys[first + cut])
        pu = float(g["u0"]) + ((cells % R) + rng.uniform(0.03, 0.97, cells.size)) * 16.0 / float(g["scale_u"])
        pv = float(g["v0"]) + ((cells // R) + rng.uniform(0.03, 0.97, cells.size)) * 16.0 / float(g["scale_v"])
        h = float(g["h_top"]) - lim
        out.append(np.outer(pu, U) / (U @ U) + np.outer(pv, V) / (V @ V) + np.outer(h, W) / (W @ W))
        aim.append(np.full(cells.size, cut))
    return np.concatenate(out), np.concatenate(aim)


def _cut_reached(im, g, o):
    """per ray: how many entries of its cell's list pass the key cut, as the kernel decides it (float32), and whether all do"""
    cell, _, _, lim = dgc.cell_of(o, g)
    keys = (im["key_word"] & np.uint32(0xffff0000)).view(F)
    cs, count = im["cell_start"], im["count"]
    passed = np.zeros(o.shape[0], np.int64)
    for k in range(6):
        ok = (count[cell] > k) & (passed == k)
        ok[ok] = keys[cs[cell[ok]] + k] <= lim[ok]
        passed += ok
    whole = (count[cell] > 0) & (keys[cs[cell] + np.maximum(count[cell], 1) - 1] <= lim)
    return passed, whole


@pytest.mark.parametrize("res", [1, 8])
@pytest.mark.parametrize("name", ["soup", "pairs", "near"])
def test_answers_where_the_parts_of_the_image_meet(hprt, orc, tmp_path, name, res):
    """Hand-built cells: the key cut in front of entry 0, 1, 2 (the block's last decision), 3 (the first the records decide) and 4 and
    behind the list; leaves of two triangles in block slots and in records ("pairs": the leaf box is gathered, and a failed box
    goes back to the block); a near list that is not empty ("near": a triangle with a vertex that is not a number — the rule)."""
    p = tmp_path / (name + ".pbrt")
    p.write_text(_seam_texts()[name])
    model = hprt.Model.parse(str(p))
    path = str(tmp_path / (name + ".hprt"))
    model.save(path)
    scene = _scene(hprt, model, res)
    info = scene.distant_grid_info()
    assert info["eligible"] and info["R"] == res and info["near"] == (1 if name == "near" else 0), info
    im = scene.distant_grid_image()
    shapes = dgc.baked_reader.read_shapes(path)
    p9 = np.concatenate([s["P"][s["indices"]].reshape(-1, 9) for s in shapes["shapes"]]).astype(F)
    w = np.array(shapes["lights"][0]["pos"], F)
    finite = p9[np.isfinite(p9).all(1)]
    g = hprt.distant_grid_build(finite, w, res)
    assert np.array_equal(info["U"], g["U"]) and np.array_equal(info["V"], g["V"])
    rng = np.random.default_rng(5)
    # ("pairs": a triangle and its twin have one key, so no cut falls between an even entry and the next)
    cuts = (0, 2, 4, -1) if name == "pairs" else CUTS
    rays = dgc.family_rays(finite, w, hprt.distant_grid_build(finite, w, 64), seed=3, n_each=1500)
    o = np.concatenate([r[0] for r in rays.values()]); d = np.concatenate([r[1] for r in rays.values()]); tm = np.concatenate([r[2] for r in rays.values()])
    n_aimed = 0
    if name != "near":      # (the image's cells hold what the host hook's do: aim through the hook's frame)
        assert np.array_equal(im["count"], np.diff(g["cell_start"].astype(np.int64)))
        q, aim = _aimed(im, g, rng, cuts)
        radius, _, _ = dgc.world_radius(finite)
        zero = np.zeros(q.shape, F)
        oa, da = dgc.form_rays(q.astype(F), zero, zero, w, radius)
        n_aimed = oa.shape[0]
        o = np.concatenate([oa, o]); d = np.concatenate([da, d]); tm = np.concatenate([np.full(n_aimed, dgc.TMAX, F), tm])
        passed, whole = _cut_reached(im, g, oa)
        assert set(aim.tolist()) == set(cuts) if res > 1 else {0, -1} <= set(aim.tolist())
        for cut in np.unique(aim):
            sel = aim == cut
            ok = whole[sel] if cut < 0 else (passed[sel] == cut)
            assert sel.sum() == 400 and ok.all(), (name, res, cut, int(ok.sum()))
    if name == "pairs":
        single = (im["prim_word"] & np.uint32(hprt.SG_SINGLE)) != 0
        slot = np.arange(single.size) - np.repeat(im["cell_start"][:-1], im["count"])
        assert (~single & (slot < 2)).sum() > 0 and (~single & (slot >= 2)).sum() > 0
    n = o.shape[0]
    assert n < 20000
    rays7 = _rays7(o, d, tm)
    walk = _walk(_scene(hprt, model, grid="0"), rays7, n)
    assert np.array_equal(walk, np.asarray(orc.OracleScene(path).occluded(o, d, tm)[0], np.uint8))
    assert 0.05 * n < walk.sum() < 0.95 * n
    got = _grid(scene, rays7, n)
    bad = np.nonzero(got != walk)[0]
    assert bad.size == 0, (name, res, bad.size, bad[:8], bad[:8] < n_aimed, o[bad[:4]], d[bad[:4]])


def _film(scene, opt=None, **kw):
    film, st = scene.render(opt, **kw)
    return film.view(np.uint32), st


def _mixed_text():
    P, idx = sgc.soup(400, 5, centre_lo=-1.5, centre_hi=1.5)
    mats = ['Material "matte" "color Kd" [.6 .5 .4]\n', 'Material "plastic" "color Kd" [.2 .4 .6] "color Ks" [.4 .4 .4] "float roughness" [.1]\n',
            'Material "mirror" "color Kr" [.9 .9 .9]\n', 'Material "glass" "float index" [1.5]\n']
    mixed = "".join(mat + sgc.mesh(P[300 * k:300 * (k + 1)], np.arange(300).reshape(-1, 3)) for k, mat in enumerate(mats))
    return dgc.scene_text(dgc.GENERIC, [sgc.floor(-2.0)], material=mats[0], spp=16, maxdepth=5, extra=mixed), (P, idx)


def _crop64(model, spp):
    """the model's options with a 64 x 64 crop near the film's centre"""
    opt = model.options.copy()
    crop = (0.42, 0.42 + 64.0 / opt.xres, 0.47, 0.47 + 64.0 / opt.yres)
    for i in range(4):
        opt.crop[i] = crop[i]
    opt.spp = spp
    return opt, crop


def test_films_with_the_grid_are_the_films_with_the_walk(hprt, orc, cases, tmp_path):
    mixed, _ = _mixed_text()
    # (the atrium is closed: under a light from outside its film is black, the answers all "occluded"; atrium_open lacks the ceiling)
    todo = {"mixed": None, "atrium": None, "atrium_open": None, "killeroo": 8, "dodecahedron": 8}
    for name, spp in todo.items():
        if name in ("mixed", "atrium_open"):
            p = tmp_path / (name + ".pbrt")
            p.write_text(mixed if name == "mixed" else dgc.atrium_text(open_roof=True))
            model = hprt.Model.parse(str(p))
        else:
            model = cases[name]["model"]
        opt, crop = _crop64(model, spp) if spp else (None, None)
        scene = _scene(hprt, model, grid=None)
        assert scene.distant_grid_info()["eligible"] and scene.distant_grid_info()["R"] == hprt.DG_DEFAULT_RES, name
        film_grid, st = _film(scene, opt)
        assert st["shadow_rays"] > 0
        launches = scene.distant_grid_info()["render_launches"]
        assert launches > 0 and scene.shadow_grid_info()["render_launches"] == 0, name
        was = hprt.debug_shadow_grid(0)
        try:
            film_walk, st_walk = _film(scene, opt)
        finally:
            hprt.debug_shadow_grid(was)
        assert scene.distant_grid_info()["render_launches"] == launches      # (switched off: the walk)
        assert st_walk["shadow_rays"] == st["shadow_rays"]
        assert np.array_equal(film_grid, film_walk), (name, int((film_grid != film_walk).any(axis=2).sum()))
        assert name == "atrium" or film_grid.view(F)[..., :3].max() > 0, name
        off = _scene(hprt, model, grid="0")      # HPRT_SHADOW_GRID=0 at scene creation: no grid, the walk
        assert not off.distant_grid_info()["eligible"]
        assert np.array_equal(_film(off, opt)[0], film_walk), name
        assert off.distant_grid_info()["render_launches"] == 0 and off.shadow_grid_info()["render_launches"] == 0, name
        # a poisoned workspace changes nothing
        scene.debug_poison(0xFF)
        try:
            assert np.array_equal(_film(scene, opt)[0], film_grid), name
        finally:
            scene.debug_poison(None)
        if spp:      # the fixtures: the oracle's film too
            oracle = orc.OracleScene(cases[name]["path"])
            oracle.set_film(crop=crop, spp=spp)
            film0 = oracle.render(spp=spp, threads=8)[1]
            assert np.array_equal(film0.view(np.uint32), film_grid), name


def test_scenes_and_renders_that_keep_the_walk_launch_nothing_on_the_grid(hprt, cases, tmp_path):
    sp, fl = sgc.soup(300, 9), sgc.floor()
    point = 'LightSource "point" "point from" [0.125 0.25 3.5] "color I" [20 20 20]\n'
    sphere = 'AttributeBegin\nTranslate 0 0 0.5\nShape "sphere" "float radius" [0.6]\nAttributeEnd\n'
    P, idx = sgc.soup(20, 10, centre_lo=-0.5, centre_hi=0.5)
    instance = ('ObjectBegin "thing"\n' + sgc.mesh(P, idx) + 'ObjectEnd\nAttributeBegin\nTranslate 1 1 1\nObjectInstance "thing"\nAttributeEnd\n')
    texts = {
        "distant + point": dgc.scene_text(dgc.GENERIC, [sp, fl], lights=dgc.light_line(dgc.GENERIC) + point),
        "two distant": dgc.scene_text(dgc.GENERIC, [sp, fl], lights=dgc.light_line(dgc.GENERIC) + dgc.light_line(dgc.AXIS_Z)),
        "distant + a sphere": dgc.scene_text(dgc.GENERIC, [sp, fl], extra=sphere),
        "distant + an instance": dgc.scene_text(dgc.GENERIC, [sp, fl], extra=instance),
    }
    for what, text in texts.items():
        p = tmp_path / "scene.pbrt"
        p.write_text(text)
        scene = _scene(hprt, hprt.Model.parse(str(p)), grid="1")
        assert not scene.distant_grid_info()["eligible"] and not scene.shadow_grid_info()["eligible"], what
        _, st = _film(scene)
        assert st["shadow_rays"] > 0 and scene.distant_grid_info()["render_launches"] == 0, what
    # an eligible scene: counting, per-pixel-statistics, ambient-occlusion and direct-lighting renders and an attached tree keep the walk
    model = cases["soup"]["model"]
    scene = _scene(hprt, model, grid=None)
    assert scene.distant_grid_info()["eligible"]
    plain, st = _film(scene)
    launches = scene.distant_grid_info()["render_launches"]
    assert launches > 0
    counted, stc = _film(scene, count_work=True)
    stats, _ = _film(scene, pixel_stats=True)
    scene.render_ao(n_samples=4)
    scene.render_direct()
    assert scene.distant_grid_info()["render_launches"] == launches
    assert np.array_equal(counted, plain) and np.array_equal(stats, plain) and stc["shadow_rays"] == st["shadow_rays"]
    scene.attach_kdtree(hprt.KdTree(model))
    _film(scene)
    assert scene.distant_grid_info()["render_launches"] == launches


@pytest.mark.parametrize("name", sorted(sgc.scenes()))
def test_point_lit_scenes_still_take_the_point_lights_grid(hprt, tmp_path, name):
    """every point-lit scene of shadow_grid_cases: the point light's grid as the host hook builds it, k_shadow_grid in the render, and
    nothing of the distant light's"""
    text, near = sgc.scenes()[name]
    p = tmp_path / "point.pbrt"
    p.write_text(text)
    scene = _scene(hprt, hprt.Model.parse(str(p)), grid="1")
    info = scene.shadow_grid_info()
    assert sorted(info) == sorted(["eligible", "R", "entries", "near", "bytes", "build_seconds", "longest", "mean", "light", "render_launches"])
    g = hprt.shadow_grid_build(sgc.text_triangles(text), sgc.text_light(text), 512)
    assert info["eligible"] and info["R"] == 512 and np.array_equal(info["light"], sgc.text_light(text)), info
    assert info["near"] == g["near"] == (3 if near == "some" else 0) and info["entries"] == g["prim"].size and info["longest"] == g["longest"], info
    assert not scene.distant_grid_info()["eligible"]
    _, st = _film(scene)
    assert st["shadow_rays"] > 0 and scene.shadow_grid_info()["render_launches"] > 0 and scene.distant_grid_info()["render_launches"] == 0


_ONE_WORKGROUP_SCRIPT = r"""
import importlib, sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
hprt = importlib.import_module("thesis-pbrt-v3_amd")
model = hprt.Model.parse(sys.argv[2]); scene = hprt.Scene(model, hprt.Bvh(model), device=0)
info = scene.distant_grid_info()
assert info["eligible"] and info["R"] == 8, info
film, _ = scene.render()
assert scene.distant_grid_info()["render_launches"] > 0      # the render's shadow rays went through k_distant_grid
np.save(sys.argv[3], film)
r = np.load(sys.argv[4])
rays7 = torch.from_numpy(r).to("cuda:0"); occ = torch.full((r.shape[1],), 7, dtype=torch.uint8, device="cuda:0")
scene.distant_grid_occluded_device(r.shape[1], rays7.data_ptr(), occ.data_ptr())
np.save(sys.argv[5], occ.cpu().numpy())
"""


def test_one_workgroup_working_through_many_queue_chunks(hprt, cases, tmp_path):
    """One workgroup (HPRT_TRACE_MAX_BLOCKS=1) and 64-ray chunks on the soup at R = 8: every wave draws chunk after chunk while its
    lanes stand in blocks and deep in the records, so a refill that kept the entry window of an exhausted chunk would show."""
    c = cases["soup"]
    p = tmp_path / "soup.pbrt"
    p.write_text(dgc.scenes()["soup"])
    n = 20000
    pick = np.random.default_rng(2).permutation(c["o"].shape[0])[:n]
    rays = str(tmp_path / "rays.npy"); film = str(tmp_path / "film.npy"); occ = str(tmp_path / "occ.npy")
    np.save(rays, np.ascontiguousarray(np.concatenate([c["o"][pick].T, c["d"][pick].T, c["tm"][pick][None, :]]).astype(F)))
    env = dict(os.environ, HPRT_TRACE_MAX_BLOCKS="1", HPRT_TRACE_CHUNK_MAX="64", HPRT_SHADOW_GRID="1", HPRT_SHADOW_GRID_RES="8")
    r = subprocess.run([sys.executable, "-c", _ONE_WORKGROUP_SCRIPT, ROOT, str(p), film, rays, occ], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(np.load(occ), c["walk"][pick])
    scene = _scene(hprt, c["model"], grid="0")
    assert np.array_equal(np.load(film).view(np.uint32), _film(scene)[0])
