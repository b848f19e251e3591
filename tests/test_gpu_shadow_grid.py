"""k_shadow_grid (csrc/device/shadow_grid.hip) on the GPU: the any-hit answers of point-light shadow rays from the
light-centred candidate grid are the walk's and the oracle's, byte for byte, and films rendered through it are the films rendered
through the walk, bit for bit.

Rays: every one ends at the scene's light — o float32, d = float32(light - o) as Interaction::SpawnRayTo forms it, tMax = 1 -
ShadowEpsilon — from origins spread over the bound, on the surfaces (offset to either side as shading offsets them), behind triangle
vertices, edge points and points a few ulps to either side of an edge (so that the ray grazes them), with directions exactly on
cell boundaries, face boundaries and cube corners of the grid, with zero direction components, and at the distance from the light
where a triangle's depth key starts to pass, a few ulps to either side.  R = 8 makes every list long, 64 and the default exercise
the margins.  These scenes are created with HPRT_SHADOW_GRID=1: by default a scene keeps the walk where its lists are too long to
beat it (R = 8; the living room, whose 190 degenerate triangles all sit in the near list)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import shadow_grid_cases as sgc
from shadow_grid_cases import grid_scene as _scene
from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import baked_reader  # noqa: E402

pytestmark = pytest.mark.gpu

SCENES = sgc.scenes()
NAMES = sorted(SCENES) + ["living_room"]
TMAX = np.float32(1) - np.float32(0.0001)


def _baked(name, tmp, hprt):
    if name == "living_room":      # (the fixture stores its textures compact; the oracle reads the expanded form)
        model = hprt.Model.load(os.path.join(GOLDEN, "living_room.hprt"))
        path = os.path.join(tmp, "living_room.hprt")
        model.save(path)
        return model, path
    p = os.path.join(tmp, name + ".pbrt")
    with open(p, "w") as f:
        f.write(SCENES[name][0])
    model = hprt.Model.parse(p)
    path = os.path.join(tmp, name + ".hprt")
    model.save(path)
    return model, path


def _ulps(x, k):
    x = np.asarray(x, np.float32).copy()
    for _ in range(abs(k)):
        x = np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf)).astype(np.float32)
    return x


def _origins(p9, L, keys, rng):
    """[n, 3] float32 origins of the families of the module docstring (~150,000)"""
    n = p9.shape[0]
    tri = p9.reshape(n, 3, 3).astype(np.float64)
    Ld = L.astype(np.float64)
    lo = np.minimum(tri.reshape(-1, 3).min(0), Ld); hi = np.maximum(tri.reshape(-1, 3).max(0), Ld)
    ext = float((hi - lo).max())
    out = []
    # spread over the bound (and a little around it)
    out.append(lo + rng.uniform(-0.05, 1.05, (40000, 3)) * (hi - lo))
    # on the surfaces, offset along the normal to either side by what an error bound of a few ulps to a visible gap gives
    t = rng.integers(0, n, 30000)
    w = rng.dirichlet((1, 1, 1), t.size)
    p = np.einsum("kv,kvc->kc", w, tri[t])
    nrm = np.cross(tri[t, 1] - tri[t, 0], tri[t, 2] - tri[t, 0])
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
    out.append(p + nrm * (rng.choice([-1.0, 1.0], (t.size, 1)) * ext * 10.0 ** rng.uniform(-7, -3, (t.size, 1))))
    # behind a vertex, an edge point, a point a few ulps to either side of an edge: the ray from there to the light grazes it
    t = rng.integers(0, n, 30000)
    kind = rng.integers(0, 3, t.size)
    a = rng.integers(0, 3, t.size); b = (a + 1) % 3
    s = np.where(kind == 0, 0.0, rng.random(t.size))[:, None]
    q = (tri[t, a] * (1 - s) + tri[t, b] * s).astype(np.float32)
    for k in range(t.size // 3):      # (a third of them: nudged across the edge by -3 .. 3 ulps of every coordinate)
        q[k] = _ulps(q[k], int(rng.integers(-3, 4)))
    q = q.astype(np.float64)
    out.append(q + (q - Ld) * rng.uniform(0.02, 1.5, (t.size, 1)))
    # directions exactly on cell boundaries (u = k / 32: a boundary at R = 8, 64 and 512), face boundaries (|u| = 1) and cube corners,
    # and with zero components: light - o is exact where the light's coordinates are short (the test scenes' lights are)
    k = 20000
    m = 2.0 ** rng.integers(-3, 2, k)
    u = rng.integers(-32, 33, k) / 32.0
    v = np.where(rng.random(k) < 0.5, rng.integers(-32, 33, k) / 32.0, rng.uniform(-1, 1, k))
    edge = rng.random(k) < 0.3
    u = np.where(edge, rng.choice([-1.0, 1.0], k), u)
    v = np.where(edge & (rng.random(k) < 0.4), rng.choice([-1.0, 1.0], k), v)      # both +-1: a cube corner
    zero = rng.random(k) < 0.25
    u = np.where(zero, 0.0, u); v = np.where(zero & (rng.random(k) < 0.5), 0.0, v)
    axis = rng.integers(0, 3, k); sign = rng.choice([-1.0, 1.0], k)
    vec = np.zeros((k, 3))
    vec[np.arange(k), axis] = sign * m; vec[np.arange(k), (axis + 1) % 3] = u * m; vec[np.arange(k), (axis + 2) % 3] = v * m
    out.append(Ld + vec)
    # at the distance where a triangle's key starts to pass: key <= |d|^2 (1 + 2^-20), a few ulps of the distance to either side
    t = rng.integers(0, n, 20000)
    c = tri[t].mean(1) - Ld
    c /= np.maximum(np.linalg.norm(c, axis=1, keepdims=True), 1e-30)
    r = np.sqrt(keys[t].astype(np.float64) / (1 + 2.0 ** -20)) * (1 + rng.integers(-6, 7, t.size) * 2.0 ** -24)
    out.append(Ld + c * r[:, None])
    return np.concatenate(out).astype(np.float32)


@pytest.fixture(scope="module")
def cases(hprt, orc, tmp_path_factory):
    """per scene: the model, the rays, and the answers of the walk and of the oracle — computed once, shared by the R's"""
    import torch
    tmp = str(tmp_path_factory.mktemp("sg"))
    out = {}
    for name in NAMES:
        model, path = _baked(name, tmp, hprt)
        shapes = baked_reader.read_shapes(path)
        assert len(shapes["lights"]) == 1 and shapes["lights"][0]["type"] == 0
        L = np.array(shapes["lights"][0]["pos"], np.float32)
        p9 = np.concatenate([s["P"][s["indices"]].reshape(-1, 9) for s in shapes["shapes"] if s["kind"] == 0]).astype(np.float32)
        keys = np.zeros(p9.shape[0], np.float32)
        g = hprt.shadow_grid_build(p9, L, 64)
        keys[g["prim"]] = g["key"]
        o = _origins(p9, L, keys, np.random.default_rng(11))
        d = (L[None, :] - o).astype(np.float32)      # SpawnRayTo: the light's position minus the (offset) origin, in float
        ok = np.isfinite(o).all(1) & (np.abs(d).max(1) > 0)
        o, d = o[ok], d[ok]
        assert o.shape[0] <= 400000
        tm = np.full(o.shape[0], TMAX, np.float32)
        walk_scene = _scene(hprt, model, grid="0")
        assert not walk_scene.shadow_grid_info()["eligible"]
        walk = walk_scene.occluded(o, d, tm)
        oracle = orc.OracleScene(path).occluded(o, d, tm)[0]
        rays7 = torch.from_numpy(np.ascontiguousarray(np.concatenate([o.T, d.T, tm[None, :]]))).to("cuda:0")
        out[name] = {"model": model, "L": L, "o": o, "d": d, "walk": walk, "oracle": oracle, "rays7": rays7}
    return out


@pytest.mark.parametrize("res", [8, 64, None])
@pytest.mark.parametrize("name", NAMES)
def test_grid_answers_are_the_walks_and_the_oracles(hprt, cases, name, res):
    import torch
    c = cases[name]
    assert np.array_equal(c["walk"], c["oracle"])
    assert 0 < int(c["walk"].sum()) < c["walk"].size
    scene = _scene(hprt, c["model"], res)
    info = scene.shadow_grid_info()
    assert info["eligible"] and np.array_equal(info["light"], c["L"]) and (res is None or info["R"] == res), info
    if name != "near":
        assert info["near"] <= 0.01 * c["model"].counts()["triangles"]
    n = c["o"].shape[0]
    occ = torch.full((n,), 7, dtype=torch.uint8, device="cuda:0")
    scene.shadow_grid_occluded_device(n, c["rays7"].data_ptr(), occ.data_ptr())
    got = occ.cpu().numpy()
    bad = np.nonzero(got != c["walk"])[0]
    assert bad.size == 0, (name, res, bad.size, bad[:8], got[bad[:8]], c["o"][bad[:4]], c["d"][bad[:4]])
    # the boundary family did put directions exactly on cell and face boundaries where the light's coordinates allow it
    if name != "living_room":
        dd = -c["d"]
        m = np.abs(dd).max(1, keepdims=True)
        assert ((np.abs(dd) == m).sum(1) >= 2).sum() > 1000 and (dd == 0).any(1).sum() > 1000


def _film(scene, opt=None):
    film, st = scene.render(opt)
    return film.view(np.uint32), st


def test_films_with_the_grid_are_the_films_with_the_walk(hprt, tmp_path):
    """atrium(0.1) at 64x64, 16 spp and a point-lit matte / plastic / mirror / glass scene take the grid; a scene with a triangle emitter and a
    scene with a quadric do not (asserted) and render as before."""
    P, idx = sgc.soup(400, 5, centre_lo=-1.5, centre_hi=1.5)
    mixed = ""
    mats = ['Material "matte" "color Kd" [.6 .5 .4]\n', 'Material "plastic" "color Kd" [.2 .4 .6] "color Ks" [.4 .4 .4] "float roughness" [.1]\n',
            'Material "mirror" "color Kr" [.9 .9 .9]\n', 'Material "glass" "float index" [1.5]\n']
    for k, mat in enumerate(mats):
        mixed += mat + sgc.mesh(P[300 * k:300 * (k + 1)], np.arange(300).reshape(-1, 3))
    L = np.array([0.125, 0.25, 3.5], np.float32)
    emitter = ('AttributeBegin\nAreaLightSource "area" "color L" [8 8 8]\n' + sgc.mesh([[-1, -1, 3.9], [1, -1, 3.9], [0, 1, 3.9]], [[0, 2, 1]]) + "AttributeEnd\n")
    quadric = 'AttributeBegin\nTranslate 0 0 0.5\nShape "sphere" "float radius" [0.6]\nAttributeEnd\n'
    texts = {
        "atrium": (SCENES["atrium"][0], True),
        "mixed": (sgc.scene_text(L, [sgc.floor(-2.0)], material=mats[0], spp=16, maxdepth=5, extra=mixed), True),
        "emitter": (sgc.scene_text(L, [sgc.floor(-2.0), (P, idx)], spp=8, extra=emitter), False),
        "quadric": (sgc.scene_text(L, [sgc.floor(-2.0), (P, idx)], spp=8, extra=quadric), False),
    }
    for name, (text, eligible) in texts.items():
        p = tmp_path / (name + ".pbrt")
        p.write_text(text)
        model = hprt.Model.parse(str(p))
        scene = _scene(hprt, model, grid=None)
        assert scene.shadow_grid_info()["eligible"] == eligible, name
        film_grid, st = _film(scene)
        assert st["shadow_rays"] > 0
        # the eligible scenes' shadow rays did go through k_shadow_grid (one launch per bounce with shadow rays), the others' did not
        launches = scene.shadow_grid_info()["render_launches"]
        assert (launches > 0) == eligible, (name, launches)
        was = hprt.debug_shadow_grid(0)
        try:
            film_walk, st_walk = _film(scene)
        finally:
            hprt.debug_shadow_grid(was)
        assert scene.shadow_grid_info()["render_launches"] == launches      # (switched off: the walk)
        assert st_walk["shadow_rays"] == st["shadow_rays"]
        assert np.array_equal(film_grid, film_walk), (name, int((film_grid != film_walk).any(axis=2).sum()))
        off = _scene(hprt, model, grid="0")      # HPRT_SHADOW_GRID=0 at scene creation: no grid, the walk
        assert not off.shadow_grid_info()["eligible"]
        assert np.array_equal(_film(off)[0], film_walk), name


_ONE_WORKGROUP_SCRIPT = r"""
import importlib, os, sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
hprt = importlib.import_module("thesis-pbrt-v3_amd")
model = hprt.Model.parse(sys.argv[2]); scene = hprt.Scene(model, hprt.Bvh(model), device=0)
assert scene.shadow_grid_info()["eligible"]
film, _ = scene.render()
assert scene.shadow_grid_info()["render_launches"] > 0      # the render's shadow rays went through k_shadow_grid
np.save(sys.argv[3], film)
r = np.load(sys.argv[4])
rays7 = torch.from_numpy(r).to("cuda:0"); occ = torch.full((r.shape[1],), 7, dtype=torch.uint8, device="cuda:0")
scene.shadow_grid_occluded_device(r.shape[1], rays7.data_ptr(), occ.data_ptr())
np.save(sys.argv[5], occ.cpu().numpy())
"""


def test_one_workgroup_working_through_many_queue_chunks(hprt, cases, tmp_path):
    """One workgroup (HPRT_TRACE_MAX_BLOCKS=1) and 64-ray chunks, as test_few_waves_working_through_many_queue_chunks: every wave draws
    chunk after chunk, so a refill that kept the entry window of an exhausted chunk would show."""
    p = tmp_path / "atrium.pbrt"
    p.write_text(SCENES["atrium"][0])
    c = cases["atrium"]
    n = 20000
    rays = str(tmp_path / "rays.npy"); film = str(tmp_path / "film.npy"); occ = str(tmp_path / "occ.npy")
    np.save(rays, np.ascontiguousarray(np.concatenate([c["o"][:n].T, c["d"][:n].T, np.full((1, n), TMAX, np.float32)])))
    env = dict(os.environ, HPRT_TRACE_MAX_BLOCKS="1", HPRT_TRACE_CHUNK_MAX="64")
    for k in ("HPRT_SHADOW_GRID", "HPRT_SHADOW_GRID_RES"):
        env.pop(k, None)      # (the default: the atrium's grid is one the cost model keeps)
    r = subprocess.run([sys.executable, "-c", _ONE_WORKGROUP_SCRIPT, ROOT, str(p), film, rays, occ], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(np.load(occ), c["walk"][:n])
    scene = _scene(hprt, hprt.Model.parse(str(p)), grid="0")
    assert np.array_equal(np.load(film).view(np.uint32), _film(scene)[0])
