"""What the distant-grid tests share (tests/test_distant_grid_host.py, tests/test_gpu_distant_grid.py): the scenes — the soups, floor and
.pbrt head of shadow_grid_cases under one LightSource "distant" each, and two fixtures of tests/golden — the shadow rays of such a light
formed in float32 operation for operation as a render forms them (kernels.hip: SpawnRayTo over light_sample's T = p + w * 2 worldRadius),
and the device's cell and key limit of an origin restated in float32 (csrc/device/distant_grid.hip)."""
import os
import re
import sys

import numpy as np

import shadow_grid_cases as sgc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import baked_reader  # noqa: E402
import scene_gen  # noqa: E402

F = np.float32
TMAX = F(1) - F(0.0001)      # 1 - ShadowEpsilon
GAMMA7 = F(7 * 2.0 ** -24 / (1 - 7 * 2.0 ** -24))
FIXTURES = ("killeroo", "dodecahedron")
MATTE = 'Material "matte" "color Kd" [.6 .6 .6]\n'


def light_line(frm):
    return 'LightSource "distant" "point from" [%.9g %.9g %.9g] "point to" [0 0 0] "color L" [3 3 3]\n' % tuple(frm)


def scene_text(frm, meshes, material=MATTE, xres=64, yres=64, spp=4, maxdepth=3, extra="", lights=None):
    body = (light_line(frm) if lights is None else lights) + material
    return sgc.HEAD % (xres, yres, spp, maxdepth) + body + "".join(sgc.mesh(P, idx) for P, idx in meshes) + extra + "WorldEnd\n"


GENERIC, AXIS_Z, GRAZING, AXIS_X = (0.4, -0.5, 1.0), (0.0, 0.0, 1.0), (1.0, 0.05, 0.08), (1.0, 0.0, 0.0)


def atrium_text(open_roof=False):
    """atrium(0.1) with its light line replaced by a distant light from above at a slant.  The hall is closed, so inside it every
    shadow ray of that light ends at the ceiling; open_roof leaves the ceiling (the one mesh that lies in z = 7) out, for a film
    with light in it"""
    text = scene_gen.atrium(0.1, xres=64, yres=64, spp=16, maxdepth=5)[0]
    line = re.search(r'LightSource "point"[^\n]*\n', text).group(0)
    text = text.replace(line, 'LightSource "distant" "point from" [0.3 -0.2 1] "point to" [0 0 0] "color L" [3 3 3]\n')
    if open_roof:
        roofs = [m.group(0) for m in re.finditer(r'Shape "trianglemesh" "integer indices" \[[^\]]*\] "point P" \[([^\]]*)\]\n', text)
                 if (np.array(m.group(1).split(), np.float64).reshape(-1, 3)[:, 2] == 7.0).all()]
        assert len(roofs) == 1
        text = text.replace(roofs[0], "")
    return text


def scenes():
    """name -> .pbrt text, one distant light each"""
    sp = sgc.soup(2000, 1)
    # two large triangles exactly in planes that contain w = (1, 0, 0): z = 0.5 and y = 0.25
    inP = np.array([[-3, -3, 0.5], [3, -3, 0.5], [0, 3, 0.5], [-3, 0.25, -3], [3, 0.25, -3], [0, 0.25, 3]], np.float32)
    # one triangle with two equal vertices and one with collinear vertices
    degP = np.array([[1, 1, 1], [1, 1, 1], [1.5, 1, 1.2], [-1, -1, 0], [-1.5, -1.5, 0.5], [-2, -2, 1]], np.float32)
    shift = np.array([900, -700, 400], np.float32)
    offP, offI = sgc.soup(500, 3, centre_lo=-2.0, centre_hi=2.0)
    flP, flI = sgc.floor()
    return {
        "soup": scene_text(GENERIC, [sp, sgc.floor()]),
        "soup_axis": scene_text(AXIS_Z, [sp, sgc.floor()]),
        "soup_grazing": scene_text(GRAZING, [sp, sgc.floor()]),
        "axis": scene_text(AXIS_X, [(inP, np.arange(6).reshape(2, 3)), sgc.soup(600, 6), sgc.floor()]),
        "degenerate": scene_text(GENERIC, [(degP, np.arange(6).reshape(2, 3)), sgc.soup(300, 2), sgc.floor()]),
        "offset": scene_text(GENERIC, [((offP + shift).astype(np.float32), offI), ((flP + shift).astype(np.float32), flI)]),
        "atrium": atrium_text(),
    }


NAMES = sorted(scenes()) + list(FIXTURES)


def bake(hprt, name, tmp):
    """(model, path of its baked form, p9 [n, 9] float32 in creation order, w float32 [3] towards the light) of a scene of scenes() or
    of a fixture"""
    if name in FIXTURES:
        path = os.path.join(GOLDEN, name + ".hprt")
        model = hprt.Model.load(path)
    else:
        p = os.path.join(tmp, name + ".pbrt")
        with open(p, "w") as f:
            f.write(scenes()[name])
        model = hprt.Model.parse(p)
        path = os.path.join(tmp, name + ".hprt")
        model.save(path)
    shapes = baked_reader.read_shapes(path)
    assert len(shapes["lights"]) == 1 and shapes["lights"][0]["type"] == 1, name
    w = np.array(shapes["lights"][0]["pos"], np.float32)
    assert all(s["kind"] == 0 for s in shapes["shapes"]), name
    p9 = np.concatenate([s["P"][s["indices"]].reshape(-1, 9) for s in shapes["shapes"]]).astype(np.float32)
    return model, path, p9, w


def world_radius(p9):
    """Scene::worldBound's bounding sphere radius as the layout computes it (float32), and the bound"""
    P = p9.reshape(-1, 3)
    lo, hi = P.min(0).astype(F), P.max(0).astype(F)
    c = ((lo + hi) / F(2)).astype(F)
    e = (c - hi).astype(F)
    r = np.sqrt(F(F(e[0] * e[0]) + F(e[1] * e[1])) + F(e[2] * e[2]), dtype=F)
    return F(r), lo, hi


def p_error(bary, tri):
    """Triangle::Intersect's pError = gamma(7) * (|b0 p0| + |b1 p1| + |b2 p2|), float32; bary [k, 3], tri [k, 3, 3]"""
    a = np.abs((bary[:, :, None].astype(F) * tri.astype(F)).astype(F))
    return (((a[:, 0] + a[:, 1]).astype(F) + a[:, 2]).astype(F) * GAMMA7).astype(F)


def _dot(a, b):
    return ((a[:, 0] * b[:, 0]).astype(F) + (a[:, 1] * b[:, 1]).astype(F) + (a[:, 2] * b[:, 2]).astype(F)).astype(F)


def form_rays(p, p_err, n, w, radius):
    """The shadow rays a render forms at the points p [k, 3] with error bounds p_err and normals n towards a distant light w:
    T = p + w * (2 worldRadius), o = OffsetRayOrigin(p, pErr, n, T - p), d = T - o; every operation in float32.  (o, d)"""
    p, p_err, n = np.asarray(p, F), np.asarray(p_err, F), np.asarray(n, F)
    w = np.broadcast_to(np.asarray(w, F), p.shape)
    T = (p + (w * F(F(2) * F(radius))).astype(F)).astype(F)
    wv = (T - p).astype(F)
    dd = _dot(np.abs(n), p_err)
    off = (dd[:, None] * n).astype(F)
    off = np.where((_dot(wv, n) < 0)[:, None], -off, off)
    po = (p + off).astype(F)
    po = np.where(off > 0, np.nextafter(po, F(np.inf)), np.where(off < 0, np.nextafter(po, F(-np.inf)), po)).astype(F)
    return po, (T - po).astype(F)


def unit_normals(tri):
    """normalised geometric normals, float32, of tri [k, 3, 3]; a degenerate triangle gets (0, 0, 1)"""
    n = np.cross(tri[:, 1].astype(np.float64) - tri[:, 0], tri[:, 2].astype(np.float64) - tri[:, 0])
    l = np.linalg.norm(n, axis=1, keepdims=True)
    return np.where(l > 0, n / np.maximum(l, 1e-300), [0.0, 0.0, 1.0]).astype(F)


def cell_of(o, g):
    """The device's cell of the origins o [k, 3] float32 (csrc/device/distant_grid.hip, DG_RAY) restated operation for operation over
    the frame of g (distant_grid_build's dict): (cell, su, sv, lim) — the cell, the sixteenth of it along u and v, the key limit"""
    o = np.asarray(o, F)
    R = g["R"]

    def proj(a):
        return ((o[:, 0] * a[0]).astype(F) + (o[:, 1] * a[1]).astype(F) + (o[:, 2] * a[2]).astype(F)).astype(F)

    def fine(pv, x0, s):
        with np.errstate(all="ignore"):
            f = np.floor(((pv - x0).astype(F) * s).astype(F))
        return np.clip(np.nan_to_num(f, nan=0.0, posinf=16 * R, neginf=-1), 0, 16 * R - 1).astype(np.int64)

    fu = fine(proj(g["U"]), g["u0"], g["scale_u"]); fv = fine(proj(g["V"]), g["v0"], g["scale_v"])
    lim = (g["h_top"] - proj(g["W"])).astype(F)
    return (fv >> 4) * R + (fu >> 4), fu & 15, fv & 15, lim


def _ulps(x, k):
    x = np.asarray(x, F).copy()
    for _ in range(abs(k)):
        x = np.nextafter(x, F(np.inf if k > 0 else -np.inf)).astype(F)
    return x


def _lowered(q, w, rng, lo_frac, hi_frac, height):
    """q moved against the light by a random share of the bound's height (a positive share: the ray from there passes through q)"""
    return q - np.asarray(w, np.float64) * (rng.uniform(lo_frac, hi_frac, (q.shape[0], 1)) * height)


def families(p9, w, g, rng, n_each=20000):
    """name -> (p, pErr, n, tMax): the shading points of the ray families of tests/test_gpu_distant_grid.py, float32, to be formed into
    rays by form_rays.  g: distant_grid_build(p9, w, 64).  Families with constructed origins carry pErr = 0, so that o = p exactly."""
    n = p9.shape[0]
    tri = p9.reshape(n, 3, 3).astype(np.float64)
    wd = np.asarray(w, np.float64)
    U, V = g["U"].astype(np.float64), g["V"].astype(np.float64)
    nrm = unit_normals(tri)
    P = tri.reshape(-1, 3)
    hs = P @ wd
    height = float(hs.max() - hs.min())
    zero = np.zeros((n_each, 3), F)
    tmax = np.full(n_each, TMAX, F)
    out = {}

    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    by_area = np.cumsum(area) / area.sum()

    def pick_triangles(k):
        """triangles as a render's hit points meet them — by area — and, for the small ones' sake, half of them one as likely as another"""
        return np.where(rng.random(k) < 0.5, rng.integers(0, n, k), np.minimum(np.searchsorted(by_area, rng.random(k)), n - 1))

    def on_triangles(k):
        t = pick_triangles(k)
        b = rng.dirichlet((1, 1, 1), k)
        return t, b, np.einsum("kv,kvc->kc", b, tri[t])

    # origins on triangles: the hit point, its error bound and the triangle's normal, to either side
    t, b, q = on_triangles(n_each)
    flip = rng.choice([-1.0, 1.0], (n_each, 1)).astype(F)
    out["surface"] = (q.astype(F), p_error(b, tri[t]), (nrm[t] * flip).astype(F), tmax)
    # cell and sixteenth boundaries: projections u0 + k / scale that the device's float expression maps exactly onto column k; exact
    # where U and V are dyadic (the axis-aligned lights), else within an ulp of the boundary
    t, b, q = on_triangles(n_each)
    q = _lowered(q, wd, rng, -0.3, 0.3, height)      # (below the point or above it)
    ku = np.floor((q @ U - float(g["u0"])) * float(g["scale_u"])); kv = np.floor((q @ V - float(g["v0"])) * float(g["scale_v"]))
    snap_u = rng.random(n_each) < 0.7; snap_v = rng.random(n_each) < 0.5
    pu = np.where(snap_u, float(g["u0"]) + ku / float(g["scale_u"]), q @ U); pv = np.where(snap_v, float(g["v0"]) + kv / float(g["scale_v"]), q @ V)
    q = q + np.outer(pu - q @ U, U) / (U @ U) + np.outer(pv - q @ V, V) / (V @ V)
    out["boundary"] = (q.astype(F), zero, zero, tmax)
    # the key seam: at the lateral position of a point of a triangle, at the height of the triangle's top, +- 0, 1, 2, 8 ulps
    t, b, q = on_triangles(n_each)
    top = (tri[t] @ wd).max(1)
    q = (q + np.outer(top - q @ wd, wd) / (wd @ wd)).astype(F)
    k = rng.choice([-8, -2, -1, 0, 1, 2, 8], n_each)
    for u in np.unique(k):
        q[k == u] = _ulps(q[k == u], int(u))
    out["seam"] = (q, zero, zero, tmax)
    # above everything, and for the other answer the same lateral spread below everything
    lo, hi = P.min(0), P.max(0)
    q = lo + rng.uniform(0.0, 1.0, (n_each, 3)) * (hi - lo)
    up = rng.random(n_each) < 0.5
    target = np.where(up, hs.max() + rng.uniform(1e-6, 0.2, n_each) * height, hs.min() - rng.uniform(1e-6, 0.2, n_each) * height)
    q = q + np.outer(target - q @ wd, wd) / (wd @ wd)
    out["above_below"] = (q.astype(F), zero, zero, tmax)
    # along edges and through vertices: points of edges (shared by two triangles where the meshes share them) and vertices, lowered
    t = pick_triangles(n_each)
    a = rng.integers(0, 3, n_each)
    s = np.where(rng.random(n_each) < 0.3, 0.0, rng.random(n_each))[:, None]
    q = tri[t, a] * (1 - s) + tri[t, (a + 1) % 3] * s
    out["edges"] = (_lowered(q, wd, rng, -0.3, 0.5, height).astype(F), zero, zero, tmax)
    # the rim: below the points of the scene that project farthest out, and from there pushed out past the rectangle (clamped cells)
    pu, pv = P @ U, P @ V
    k = max(4, min(200, P.shape[0] // 8))
    far = np.concatenate([np.argsort(pu)[:k], np.argsort(pu)[-k:], np.argsort(pv)[:k], np.argsort(pv)[-k:]])
    pick = far[rng.integers(0, far.size, n_each)]
    tq, vq = pick // 3, pick % 3
    bb = rng.dirichlet((1, 1, 1), n_each) * 0.05
    bb[np.arange(n_each), vq] += 0.95
    q = _lowered(np.einsum("kv,kvc->kc", bb, tri[tq]), wd, rng, 0.0, 0.2, height)
    centre = np.array([0.5 * (pu.min() + pu.max()), 0.5 * (pv.min() + pv.max())])
    side = np.array([pu.max() - pu.min(), pv.max() - pv.min()])
    outward = np.stack([q @ U - centre[0], q @ V - centre[1]], 1)
    outward /= np.maximum(np.abs(outward).max(1, keepdims=True), 1e-30)
    push = np.where(rng.random(n_each) < 0.5, 0.0, rng.uniform(0.0, 0.1, n_each))[:, None] * side
    q = q + np.outer(outward[:, 0] * push[:, 0], U) / (U @ U) + np.outer(outward[:, 1] * push[:, 1], V) / (V @ V)
    out["rim"] = (q.astype(F), zero, zero, tmax)
    # tMax > 1: surface rays that may run on past T
    t, b, q = on_triangles(n_each)
    out["long"] = (q.astype(F), p_error(b, tri[t]), nrm[t], rng.choice([1.0, 1.5, 4.0], n_each).astype(F) + F(2.0 ** -10))
    return out


def family_rays(p9, w, g, seed=11, n_each=20000):
    """name -> (o, d, tMax) float32 of families(); rays whose direction is not finite or zero are dropped"""
    radius, _, _ = world_radius(p9)
    out = {}
    for name, (p, pe, nn, tm) in families(p9, w, g, np.random.default_rng(seed), n_each).items():
        o, d = form_rays(p, pe, nn, w, radius)
        ok = np.isfinite(o).all(1) & np.isfinite(d).all(1) & (np.abs(d).max(1) > 0)
        out[name] = (o[ok], d[ok], tm[ok])
    return out
