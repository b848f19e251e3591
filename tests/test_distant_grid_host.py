"""The light-aligned shadow grid of a distant light (csrc/distant_grid.cpp), built on the host through
hprt_debug_distant_grid_build — no GPU.

The claim: if the device's tri_test reports a hit for a shadow ray a render forms for this light, the triangle is in the near list, or
in the list of the cell the kernel computes from the ray's origin, with a key that passes and a rectangle that holds the ray's
sixteenth.  Checked by sampling: 64 points per triangle; from each a ray as the renderer forms it (tests/distant_grid_cases.py,
form_rays: float32, operation for operation) with its origin on the triangle, and lower against the light by 0.1 and 0.9 of the
bound's height where that stays inside the bound; and the same with the point moved by the build's ε along each axis, either way.
(Every triangle of every scene; a large scene's rays are formed and looked up 4,000 triangles at a time.)
Lists, the device image, the point light's grid against a digest recorded on the parent commit, and eligibility follow."""
import hashlib
import os

import numpy as np
import pytest

import distant_grid_cases as dgc
import shadow_grid_cases as sgc

RES = (8, 64, None)      # None: the default, hprt.DG_DEFAULT_RES
F = np.float32


@pytest.fixture(scope="module")
def baked(hprt, tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("dg"))
    return {name: dgc.bake(hprt, name, tmp) for name in dgc.NAMES}


def _claim_rays(p9, w, eps, who):
    """(origins float32 [k, 3], triangle of each) of the rays of the module docstring from the triangles `who`"""
    n = p9.shape[0]
    tri = p9.reshape(n, 3, 3).astype(np.float64)[who]
    bary = sgc.triangle_points()
    pts = np.einsum("kv,nvc->nkc", bary, tri).reshape(-1, 3)
    who = np.repeat(who, bary.shape[0])
    b = np.tile(bary, (tri.shape[0], 1))
    t3 = np.repeat(tri, bary.shape[0], axis=0)
    nrm = dgc.unit_normals(t3)
    radius, lo, hi = dgc.world_radius(p9)
    wd = w.astype(np.float64)
    P = p9.reshape(-1, 3).astype(np.float64)
    height = float((P @ wd).max() - (P @ wd).min())
    moves = np.concatenate([np.zeros((1, 3)), eps * np.eye(3), -eps * np.eye(3)])
    origins, whos = [], []
    for share in (0.0, 0.1, 0.9):
        q = pts - wd * (share * height)
        keep = np.ones(q.shape[0], bool) if share == 0.0 else ((q >= lo) & (q <= hi)).all(1)
        for mv in moves:
            p = (q[keep] + mv).astype(F)
            # a hit's error bound on the triangle; gamma(7) |p| for a point in space
            pe = dgc.p_error(b[keep], t3[keep]) if share == 0.0 else (np.abs(p) * dgc.GAMMA7).astype(F)
            o, d = dgc.form_rays(p, pe, nrm[keep], w, radius)
            assert np.isfinite(d).all() and (d @ w > 0).all()
            origins.append(o); whos.append(who[keep])
    return np.concatenate(origins), np.concatenate(whos)


@pytest.mark.parametrize("name", dgc.NAMES)
def test_every_ray_from_a_triangle_finds_it_in_its_cell(hprt, baked, name):
    _, _, p9, w = baked[name]
    n = p9.shape[0]
    eps = hprt.distant_grid_build(p9, w, 8)["eps"]
    tables = []
    for R in RES:
        R = hprt.DG_DEFAULT_RES if R is None else R
        g = hprt.distant_grid_build(p9, w, R)
        assert g["R"] == R and g["eps"] == eps and np.array_equal(g["W"], w)
        in_near = np.zeros(n, bool)
        in_near[g["prim"][:g["near"]]] = True
        cs = g["cell_start"].astype(np.int64)
        cell_of_entry = np.searchsorted(cs, np.arange(g["near"], g["prim"].size), side="right") - 1
        pair = cell_of_entry * n + g["prim"][g["near"]:]
        order = np.argsort(pair)
        pair, key, rect = pair[order], g["key"][g["near"]:][order], g["rect"][g["near"]:][order]
        assert np.all(np.diff(pair) > 0)                                                # a triangle appears once in a cell
        tables.append((R, g, in_near, pair, key, rect))
    seen = 0
    for first in range(0, n, 4000):
        chunk = np.arange(first, min(n, first + 4000))
        o, who = _claim_rays(p9, w, eps, chunk)
        assert o.shape[0] >= 64 * 7 * chunk.size and np.array_equal(np.unique(who), chunk)
        seen += chunk.size
        for R, g, in_near, pair, key, rect in tables:
            cell, su, sv, lim = dgc.cell_of(o, g)
            want = cell * n + who
            at = np.minimum(np.searchsorted(pair, want), pair.size - 1)
            found = pair[at] == want
            r = rect[at]
            reached = (r[:, 0] <= su) & (su <= r[:, 1]) & (r[:, 2] <= sv) & (sv <= r[:, 3])
            ok = in_near[who] | (found & reached & (key[at] <= lim))                    # (float32 against float32, as the kernel compares)
            assert ok.all(), (name, R, int((~ok).sum()), who[~ok][:5], o[~ok][:2], found[~ok][:5], reached[~ok][:5])
    assert seen == n


@pytest.mark.parametrize("name", dgc.NAMES)
def test_lists_are_sorted_within_capacity_and_the_near_list_is_empty(hprt, baked, name):
    _, _, p9, w = baked[name]
    for R in RES:
        R = hprt.DG_DEFAULT_RES if R is None else R
        g = hprt.distant_grid_build(p9, w, R)
        cs = g["cell_start"].astype(np.int64)
        assert cs.size == R * R + 1 and cs[0] == g["near"] and cs[-1] == g["prim"].size and np.all(np.diff(cs) >= 0)
        assert int(np.diff(cs).max()) == g["longest"] and g["prim"].size < (1 << 27)
        k = g["key"]
        assert np.all(k >= 0) and np.all(np.isfinite(k))
        assert np.all(g["rect"][:, 0] <= g["rect"][:, 1]) and np.all(g["rect"][:, 2] <= g["rect"][:, 3])
        rising = np.diff(k[g["near"]:]) >= 0
        starts = cs[1:-1] - g["near"] - 1                                               # the step from one cell's last entry to the next cell's first
        rising[starts[(starts >= 0) & (starts < rising.size)]] = True
        assert rising.all()
        assert g["single"].all() and g["prim"].max() < p9.shape[0]
        # the rule: only a triangle that is not finite goes to the near list — no scene here has one; the "degenerate" scene's
        # triangle with two equal vertices (0) and its collinear one (1) lie in cells, as a segment's widened rectangle
        assert g["near"] == 0
        if name == "degenerate":
            assert (g["prim"] == 0).sum() >= 1 and (g["prim"] == 1).sum() >= 1
        # every triangle is listed somewhere
        assert np.unique(g["prim"]).size == p9.shape[0]


def test_a_triangle_that_is_not_finite_goes_to_the_near_list_and_nothing_else_does(hprt, baked):
    _, _, p9, w = baked["degenerate"]
    bad = p9.copy()
    bad[5, 4] = np.nan
    bad[17, 0] = np.inf
    lo, hi = p9.reshape(-1, 3).min(0), p9.reshape(-1, 3).max(0)
    for R in (8, 64):
        g = hprt.distant_grid_build(bad, w, R, bound=np.concatenate([lo, hi]))
        ref = hprt.distant_grid_build(p9, w, R, bound=np.concatenate([lo, hi]))
        assert g["near"] == 2 and sorted(g["prim"][:2].tolist()) == [5, 17]
        assert np.all(g["key"][:2] == 0) and np.all(g["rect"][:2] == [0, 15, 0, 15])
        assert not np.isin(g["prim"][2:], [5, 17]).any()
        # the other triangles' entries are what they are without the two
        keep = ~np.isin(ref["prim"], [5, 17])
        assert np.array_equal(g["prim"][2:], ref["prim"][keep]) and np.array_equal(g["key"][2:], ref["key"][keep]) and np.array_equal(g["rect"][2:], ref["rect"][keep])


def test_the_frame_is_orthogonal_and_dyadic_under_axis_aligned_lights(hprt, baked):
    for name in dgc.NAMES:
        _, _, p9, w = baked[name]
        g = hprt.distant_grid_build(p9, w, 8)
        U, V, W = (g[k].astype(np.float64) for k in "UVW")
        assert abs(U @ V) < 1e-6 and abs(U @ W) < 1e-6 and abs(V @ W) < 1e-6
        assert abs(U @ U - 1) < 1e-6 and abs(V @ V - 1) < 1e-6
        assert np.dot(np.cross(U, V), W) > 0.99
        # the rectangle holds the projection of every vertex, with the margin to spare
        P = p9.reshape(-1, 3).astype(np.float64)
        for a, x0, s in ((U, g["u0"], g["scale_u"]), (V, g["v0"], g["scale_v"])):
            f = (P @ a - float(x0)) * float(s)
            assert f.min() > 0 and f.max() < 16 * 8
    for name in ("soup_axis", "axis", "dodecahedron"):
        g = hprt.distant_grid_build(baked[name][2], baked[name][3], 8)
        assert set(np.abs(np.concatenate([g["U"], g["V"], g["W"]])).tolist()) == {0.0, 1.0}, name


def _logical_words(g, hprt):
    prim = (g["prim"].astype(np.uint32) | np.where(g["single"], np.uint32(hprt.SG_SINGLE), np.uint32(0))).astype(np.uint32)
    r = g["rect"].astype(np.uint32)
    key = (g["key"].view(np.uint32) | r[:, 0] | (r[:, 1] << 4) | (r[:, 2] << 8) | (r[:, 3] << 12)).astype(np.uint32)
    return prim, key


@pytest.mark.parametrize("R", (1, 8, 64))
@pytest.mark.parametrize("name", ["soup", "axis", "degenerate", "dodecahedron"])
def test_decoding_every_cell_of_the_image_gives_the_logical_list(hprt, baked, name, R):
    _, _, p9, w = baked[name]
    g = hprt.distant_grid_build(p9, w, R)
    im = hprt.distant_grid_image(p9, w, R)
    prim, key = _logical_words(g, hprt)
    cs = g["cell_start"].astype(np.int64)
    assert im["blocks"].shape == (R * R, hprt.SG_BLOCK_WORDS)
    assert np.array_equal(im["count"], np.diff(cs)) and np.array_equal(im["cell_start"], cs)
    assert np.array_equal(im["prim_word"], prim) and np.array_equal(im["key_word"], key)
    assert np.array_equal(im["verts"], p9.view(np.uint32)[g["prim"]])
    # one run of records per cell past its block, in cell order, and one record of zeros behind the last
    over = np.maximum(im["count"] - hprt.SG_BLOCK_SLOTS, 0)
    assert np.array_equal(im["overflow"][over > 0], (g["near"] + np.cumsum(over) - over)[over > 0])
    n_records = g["near"] + int(over.sum())
    assert im["records"].shape[0] == n_records + 1 and not im["records"][n_records:].any()
    has3 = im["count"] > 2
    assert np.array_equal(im["key2"][has3], key[cs[:-1][has3] + 2]) and not im["key2"][~has3].any()
    # no read the kernel can form leaves the image: seven words of the last block, three of the last record, below 2^32 bytes
    assert im["words"] == (im["blocks"].size, im["records"].size, im["blocks"].size + im["records"].size)
    assert 4 * im["blocks"].size == R * R * 128 and 4 * (im["blocks"].size + im["records"].size) < 2 ** 32
    if R == 1:
        assert im["count"][0] == p9.shape[0]


# sha256 over cell_start, prim, single, key, rect (shadow_grid_build) and blocks, records (shadow_grid_image) of
# shadow_grid_cases.scenes()["soup"], taken on the parent commit
POINT_GRID_DIGESTS = {8: "0814bff572c95cb96fe205f37837fe7016ea745633a870568e7a2eefab8b93db",
                      64: "7da147751ea77afec33ebe25d54de4d41d44d3efa66b6b736f6b55fa150a9cda"}


@pytest.mark.parametrize("R", sorted(POINT_GRID_DIGESTS))
def test_the_point_lights_grid_is_what_it_was(hprt, R):
    text = sgc.scenes()["soup"][0]
    p9, L = sgc.text_triangles(text), sgc.text_light(text)
    g, im = hprt.shadow_grid_build(p9, L, R), hprt.shadow_grid_image(p9, L, R)
    h = hashlib.sha256()
    for a in (g["cell_start"], g["prim"], g["single"], g["key"], g["rect"], im["blocks"], im["records"]):
        h.update(np.ascontiguousarray(a).tobytes())
    assert h.hexdigest() == POINT_GRID_DIGESTS[R]
    assert im["blocks"].shape[0] == 6 * R * R


def _layout(hprt, text, tmp_path, env=None):
    p = tmp_path / "scene.pbrt"
    p.write_text(text)
    model = hprt.Model.parse(str(p))
    keys = ("HPRT_SHADOW_GRID", "HPRT_SHADOW_GRID_RES", "HPRT_SHADOW_GRID_MAX_MB")
    old = {k: os.environ.pop(k, None) for k in keys}
    try:
        os.environ.update(env or {})
        return hprt.shadow_grid_layout(model, hprt.Bvh(model))
    finally:
        for k in keys:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def test_eligibility(hprt, tmp_path):
    sp, fl = sgc.soup(300, 9), sgc.floor()
    one = dgc.scene_text(dgc.GENERIC, [sp, fl])
    got = _layout(hprt, one, tmp_path)
    assert got["distant"]["eligible"] and got["distant"]["R"] == hprt.DG_DEFAULT_RES and not got["point"]["eligible"]
    assert got["distant"]["near"] == 0 and got["distant"]["bytes"] >= hprt.DG_DEFAULT_RES ** 2 * 128
    assert _layout(hprt, one, tmp_path, {"HPRT_SHADOW_GRID_RES": "64"})["distant"]["R"] == 64
    # the cap halves R until the image fits: 16 MB hold 256^2 blocks of 128 bytes and the records, not 512^2
    assert _layout(hprt, one, tmp_path, {"HPRT_SHADOW_GRID_MAX_MB": "16"})["distant"]["R"] == 256
    # R = 2 makes lists longer than the cost model takes (302 triangles in four cells): dropped by default, kept when forced
    assert not _layout(hprt, one, tmp_path, {"HPRT_SHADOW_GRID_RES": "2"})["distant"]["eligible"]
    assert _layout(hprt, one, tmp_path, {"HPRT_SHADOW_GRID_RES": "2", "HPRT_SHADOW_GRID": "1"})["distant"]["eligible"]
    point = 'LightSource "point" "point from" [0.125 0.25 3.5] "color I" [20 20 20]\n'
    sphere = 'AttributeBegin\nTranslate 0 0 0.5\nShape "sphere" "float radius" [0.6]\nAttributeEnd\n'
    P, idx = sgc.soup(20, 10, centre_lo=-0.5, centre_hi=0.5)
    instance = ('ObjectBegin "thing"\n' + sgc.mesh(P, idx) + 'ObjectEnd\nAttributeBegin\nTranslate 1 1 1\nObjectInstance "thing"\nAttributeEnd\n')
    not_eligible = {
        "distant + point": dgc.scene_text(dgc.GENERIC, [sp, fl], lights=dgc.light_line(dgc.GENERIC) + point),
        "two distant": dgc.scene_text(dgc.GENERIC, [sp, fl], lights=dgc.light_line(dgc.GENERIC) + dgc.light_line(dgc.AXIS_Z)),
        "distant + a sphere": dgc.scene_text(dgc.GENERIC, [sp, fl], extra=sphere),
        "distant + an instance": dgc.scene_text(dgc.GENERIC, [sp, fl], extra=instance),
    }
    for what, text in not_eligible.items():
        for mode in (None, "1"):
            got = _layout(hprt, text, tmp_path, {} if mode is None else {"HPRT_SHADOW_GRID": mode})
            assert not got["distant"]["eligible"] and not got["point"]["eligible"], (what, mode)
    assert not _layout(hprt, one, tmp_path, {"HPRT_SHADOW_GRID": "0"})["distant"]["eligible"]
    # a point-lit scene still gets the point light's grid, and no other
    got = _layout(hprt, sgc.scene_text(np.array([0.125, 0.25, 3.5], np.float32), [sp, fl]), tmp_path)
    assert got["point"]["eligible"] and got["point"]["R"] == 512 and not got["distant"]["eligible"]


@pytest.mark.parametrize("name", dgc.NAMES)
def test_the_ray_families_leave_neither_answer_untested(hprt, orc, baked, name):
    """A condition on the inputs of tests/test_gpu_distant_grid.py: the oracle's any-hit reports between 5 % and 95 % of every family's
    rays occluded."""
    _, path, p9, w = baked[name]
    oracle = orc.OracleScene(path)
    rays = dgc.family_rays(p9, w, hprt.distant_grid_build(p9, w, 64))
    assert sorted(rays) == sorted(["surface", "boundary", "seam", "above_below", "edges", "rim", "long"])
    for family, (o, d, tm) in rays.items():
        assert o.shape[0] >= 19000 and (d @ w > 0).all(), (name, family, o.shape[0])
        share = float(np.asarray(oracle.occluded(o, d, tm)[0]).mean())
        assert 0.05 <= share <= 0.95, (name, family, share)
        assert (tm > 1).all() if family == "long" else (tm <= 1).all()
