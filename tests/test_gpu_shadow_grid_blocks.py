"""k_shadow_grid on the grid's device image (csrc/shadow_grid.h, ShadowGridImage) where the image's parts meet: the
block's two slots, the block's copy of the third entry's key word, the first record of a cell's run, the end of a list, the near
list's run in front of everything — and leaves of two triangles, whose box is gathered after a reported hit from a block slot and
from a record.  The answers are the walk's (hprt_occluded_device on a scene without a grid) and the oracle's, byte for byte, on
every ray.

Scenes: tests/shadow_grid_cases.py's "soup", "near" (a near list of three) and "inplane", and "pairs": a soup in which every
triangle lies in the scene twice, the second time with its vertices rotated — equal bounds, equal centroids, so no BVH build can part
the two and every such leaf holds two triangles.  R = 1 (six lists, each far past a block) and R = 8.
Rays (every one ends at the light, d = float32(light - o), tMax = 1 - ShadowEpsilon):
 - aimed: from the decoded image, cells with at least four entries; directions spread inside the cell, and the origin at the
   distance from the light at which the key cut falls in front of entry 0, 1, 2 (the block's last decision), 3 (the first the
   records decide) and 4, and just behind the list's last key;
 - at the two-triangle leaves: from behind the centroid of every entry without the SG_SINGLE mark, in a block slot or in a record;
 - spread over the bound and on the surfaces, offset to either side."""
import os
import subprocess
import sys

import numpy as np
import pytest

import shadow_grid_cases as sgc
from shadow_grid_cases import grid_scene as _scene
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import baked_reader  # noqa: E402

pytestmark = pytest.mark.gpu

TMAX = np.float32(1) - np.float32(0.0001)
RES = (1, 8)
L0 = np.array([0.125, 0.25, 0.375], np.float32)
CUTS = (0, 1, 2, 3, 4, -1)      # the entry in front of which the key cut falls; -1: behind the list's last key


def _texts():
    s = sgc.scenes()
    P, idx = sgc.soup(150, 21, centre_lo=-2.5, centre_hi=2.5, size=0.5)
    twice = np.concatenate([idx, idx[:, [1, 2, 0]]])
    return {"soup": s["soup"][0], "near": s["near"][0], "inplane": s["inplane"][0], "pairs": sgc.scene_text(L0, [(P, twice), sgc.floor()])}


TEXTS = _texts()
NAMES = sorted(TEXTS)


def _cell_directions(cells, R, rng):
    """a direction (light -> point, major component 1) inside each of `cells`, away from the cell's border"""
    face, iv, iu = cells // (R * R), (cells // R) % R, cells % R
    u = (iu + rng.uniform(0.03, 0.97, cells.size)) / R * 2 - 1
    v = (iv + rng.uniform(0.03, 0.97, cells.size)) / R * 2 - 1
    axis = face // 2
    vec = np.zeros((cells.size, 3))
    k = np.arange(cells.size)
    vec[k, axis] = np.where(face % 2 == 1, -1.0, 1.0); vec[k, (axis + 1) % 3] = u; vec[k, (axis + 2) % 3] = v
    return vec


def _aimed(im, R, L, rng, cuts):
    """origins whose key cut falls at the entries of `cuts`, and the cut each was aimed at"""
    keys = (im["key_word"] & np.uint32(0xffff0000)).view(np.float32).astype(np.float64)
    cs, count = im["cell_start"], im["count"]
    out, aim = [], []
    for cut in cuts:
        # the cells whose lists can be cut there: entries cut - 1 and cut exist and their (16-bit) keys differ
        cells = np.nonzero(count >= max(1, cut + 1))[0]
        if cut > 0:
            cells = cells[keys[cs[cells] + cut - 1] < keys[cs[cells] + cut]]
        elif cut == 0:
            cells = cells[keys[cs[cells]] > 0]
        assert cells.size > 0, cut
        cells = rng.permutation(np.repeat(cells, -(-400 // cells.size)))[:400]
        vec = _cell_directions(cells, R, rng)
        first = cs[cells]
        if cut == 0:
            r2 = keys[first] * 0.9
        elif cut < 0:
            r2 = keys[first + count[cells] - 1] * 1.1 + 1e-3
        else:
            r2 = 0.5 * (keys[first + cut - 1] + keys[first + cut])
        # |d|^2 = r2: the point at that distance along the direction
        out.append(L.astype(np.float64) + vec * np.sqrt(r2 / (vec * vec).sum(1))[:, None])
        aim.append(np.full(cells.size, cut))
    return np.concatenate(out), np.concatenate(aim)


def _cut_reached(im, R, d):
    """per ray: how many entries of its cell's list pass the key cut, as the kernel decides it (float32)"""
    d = d.astype(np.float32)
    dist2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(np.float32) + d[:, 2] * d[:, 2]
    lim = (dist2 * np.float32(1 + 2.0 ** -20)).astype(np.float32)
    cell, _, _ = sgc.cell_of(d, R)
    keys = (im["key_word"] & np.uint32(0xffff0000)).view(np.float32)
    cs, count = im["cell_start"], im["count"]
    passed = np.zeros(d.shape[0], np.int64)
    for k in range(6):
        has = count[cell] > k
        ok = has & (passed == k)
        ok[ok] = keys[cs[cell[ok]] + k] <= lim[ok]
        passed += ok
    whole = (count[cell] > 0) & (keys[cs[cell] + np.maximum(count[cell], 1) - 1] <= lim)      # (keys ascend: the last passes, all do)
    return passed, whole


def _behind_unmarked(im, hprt, L, rng):
    """origins behind the centroids of the entries without the SG_SINGLE mark: (from block slots, from records)"""
    single = (im["prim_word"] & np.uint32(hprt.SG_SINGLE)) != 0
    cs = im["cell_start"]
    entry = np.arange(im["prim_word"].size)
    cell = np.searchsorted(cs, entry, side="right") - 1
    in_list = entry >= cs[0]
    slot = entry - cs[np.maximum(cell, 0)]
    out = []
    for pick in (in_list & ~single & (slot < 2), in_list & ~single & (slot >= 2)):
        at = np.nonzero(pick)[0]
        assert at.size > 0
        at = at[rng.permutation(at.size)[:600]]
        c = im["verts"][at].view(np.float32).reshape(-1, 3, 3).astype(np.float64).mean(1)
        out.append(c + (c - L.astype(np.float64)) * rng.uniform(0.05, 0.5, (at.size, 1)))
    return out


def _spread(p9, L, rng):
    tri = p9.reshape(-1, 3, 3).astype(np.float64)
    Ld = L.astype(np.float64)
    lo = np.minimum(tri.reshape(-1, 3).min(0), Ld); hi = np.maximum(tri.reshape(-1, 3).max(0), Ld)
    ext = float((hi - lo).max())
    a = lo + rng.uniform(-0.05, 1.05, (1500, 3)) * (hi - lo)
    t = rng.integers(0, tri.shape[0], 1500)
    w = rng.dirichlet((1, 1, 1), t.size)
    p = np.einsum("kv,kvc->kc", w, tri[t])
    nrm = np.cross(tri[t, 1] - tri[t, 0], tri[t, 2] - tri[t, 0])
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
    b = p + nrm * (rng.choice([-1.0, 1.0], (t.size, 1)) * ext * 10.0 ** rng.uniform(-7, -3, (t.size, 1)))
    return np.concatenate([a, b])


@pytest.fixture(scope="module")
def cases(hprt, orc, tmp_path_factory):
    """per scene: the grid scenes of RES with their decoded images, the rays (aimed through both images, so that both R's meet all of
    them), and the answers of the walk and of the oracle — computed once"""
    import torch
    tmp = str(tmp_path_factory.mktemp("sgb"))
    out = {}
    for name in NAMES:
        p = os.path.join(tmp, name + ".pbrt")
        with open(p, "w") as f:
            f.write(TEXTS[name])
        model = hprt.Model.parse(p)
        path = os.path.join(tmp, name + ".hprt")
        model.save(path)
        shapes = baked_reader.read_shapes(path)
        L = np.array(shapes["lights"][0]["pos"], np.float32)
        p9 = np.concatenate([s["P"][s["indices"]].reshape(-1, 9) for s in shapes["shapes"] if s["kind"] == 0]).astype(np.float32)
        rng = np.random.default_rng(5)
        # ("pairs": a triangle and its twin have one key, so no cut falls between an even entry and the next)
        cuts = (0, 2, 4, -1) if name == "pairs" else CUTS
        grids, origins, aim = {}, [_spread(p9, L, rng)], {}
        for R in RES:
            scene = _scene(hprt, model, R, "1")
            info = scene.shadow_grid_info()
            assert info["eligible"] and info["R"] == R, info
            im = scene.shadow_grid_image()
            grids[R] = (scene, im, info)
            o, a = _aimed(im, R, L, rng, cuts)
            at = sum(x.shape[0] for x in origins)
            aim[R] = (at, a)
            origins.append(o)
            if name == "pairs":
                origins += _behind_unmarked(im, hprt, L, rng)
        o = np.concatenate(origins).astype(np.float32)
        d = (L[None, :] - o).astype(np.float32)
        assert np.isfinite(o).all() and (np.abs(d).max(1) > 0).all() and o.shape[0] < 20000
        tm = np.full(o.shape[0], TMAX, np.float32)
        rays7 = torch.from_numpy(np.ascontiguousarray(np.concatenate([o.T, d.T, tm[None, :]]))).to("cuda:0")
        walk_scene = _scene(hprt, model, None, "0")
        assert not walk_scene.shadow_grid_info()["eligible"]
        occ = torch.full((o.shape[0],), 7, dtype=torch.uint8, device="cuda:0")
        walk_scene.occluded_device(o.shape[0], rays7.data_ptr(), occ.data_ptr())
        torch.cuda.synchronize()
        oracle = orc.OracleScene(path).occluded(o, d, tm)[0]
        out[name] = {"grids": grids, "aim": aim, "o": o, "d": d, "rays7": rays7, "walk": occ.cpu().numpy(), "oracle": oracle, "text": p, "L": L}
    return out


@pytest.mark.parametrize("res", RES)
@pytest.mark.parametrize("name", NAMES)
def test_answers_are_the_walks_and_the_oracles(hprt, cases, name, res):
    import torch
    c = cases[name]
    scene, im, info = c["grids"][res]
    assert np.array_equal(c["walk"], np.asarray(c["oracle"], np.uint8))
    assert 0 < int(c["walk"].sum()) < c["walk"].size
    assert info["near"] == (3 if name == "near" else 0)
    n = c["o"].shape[0]
    occ = torch.full((n,), 7, dtype=torch.uint8, device="cuda:0")
    scene.shadow_grid_occluded_device(n, c["rays7"].data_ptr(), occ.data_ptr())
    got = occ.cpu().numpy()
    bad = np.nonzero(got != c["walk"])[0]
    assert bad.size == 0, (name, res, bad.size, bad[:8], got[bad[:8]], c["o"][bad[:4]], c["d"][bad[:4]])
    # the aimed rays did cut their lists where they were aimed: in front of entry 0, 1, 2, 3 and 4, and nowhere
    at, aim = c["aim"][res]
    passed, whole = _cut_reached(im, res, c["d"][at:at + aim.size])
    assert set(aim.tolist()) == set(CUTS) or name == "pairs"
    for cut in np.unique(aim):
        sel = aim == cut
        ok = whole[sel] if cut < 0 else (passed[sel] == cut)
        assert sel.sum() == 400 and ok.all(), (name, res, cut, int(ok.sum()), int(sel.sum()))


def test_two_triangle_leaves_are_met_in_blocks_and_in_records(hprt, cases):
    """the "pairs" scene: entries without the SG_SINGLE mark stand in block slots and in records, and rays from behind them are
    occluded — their reported hits went through the gathered leaf box (the answers themselves: the test above)"""
    c = cases["pairs"]
    for res in RES:
        _, im, _ = c["grids"][res]
        single = (im["prim_word"] & np.uint32(hprt.SG_SINGLE)) != 0
        slot = np.arange(single.size) - np.repeat(im["cell_start"][:-1], im["count"])
        assert (~single & (slot < 2)).sum() > 0 and (~single & (slot >= 2)).sum() > 0
        assert (~single).sum() >= 0.5 * single.size      # (every soup triangle's leaf holds its twin too)
    assert c["walk"].sum() > 1000


_ONE_WORKGROUP_SCRIPT = r"""
import importlib, sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
hprt = importlib.import_module("thesis-pbrt-v3_amd")
model = hprt.Model.parse(sys.argv[2]); scene = hprt.Scene(model, hprt.Bvh(model), device=0)
info = scene.shadow_grid_info()
assert info["eligible"] and info["R"] == 1 and info["near"] == 3, info
r = np.load(sys.argv[3])
rays7 = torch.from_numpy(r).to("cuda:0"); occ = torch.full((r.shape[1],), 7, dtype=torch.uint8, device="cuda:0")
scene.shadow_grid_occluded_device(r.shape[1], rays7.data_ptr(), occ.data_ptr())
np.save(sys.argv[4], occ.cpu().numpy())
"""


def test_one_workgroup_working_through_many_queue_chunks(cases, tmp_path):
    """One workgroup (HPRT_TRACE_MAX_BLOCKS=1) and 64-ray chunks on the "near" scene at R = 1: every wave draws chunk after chunk while
    its lanes stand in the near list, in blocks and deep in the records."""
    c = cases["near"]
    n = c["o"].shape[0]
    rays = str(tmp_path / "rays.npy"); occ = str(tmp_path / "occ.npy")
    np.save(rays, np.ascontiguousarray(np.concatenate([c["o"].T, c["d"].T, np.full((1, n), TMAX, np.float32)])))
    env = dict(os.environ, HPRT_TRACE_MAX_BLOCKS="1", HPRT_TRACE_CHUNK_MAX="64", HPRT_SHADOW_GRID="1", HPRT_SHADOW_GRID_RES="1")
    r = subprocess.run([sys.executable, "-c", _ONE_WORKGROUP_SCRIPT, ROOT, c["text"], rays, occ], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(np.load(occ), c["walk"])
