"""What the shadow-grid tests share (tests/test_shadow_grid_host.py, tests/test_gpu_shadow_grid.py): the scenes — .pbrt text with one
point light and untransformed triangle meshes, so that the triangles can be read back from the text — the device's cell of a
direction restated in float32, and the points on a triangle that the coverage checks use."""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import scene_gen  # noqa: E402

HEAD = ('LookAt 0 -6 2  0 0 0.5  0 0 1\nCamera "perspective" "float fov" [45]\n'
        'Film "image" "integer xresolution" [%d] "integer yresolution" [%d]\nSampler "halton" "integer pixelsamples" [%d]\n'
        'Integrator "path" "integer maxdepth" [%d]\nAccelerator "bvh"\nWorldBegin\n')


def mesh(P, idx):
    return ('Shape "trianglemesh" "integer indices" [' + " ".join(str(int(v)) for v in np.asarray(idx).ravel()) + '] "point P" [' +
            " ".join("%.9g" % v for v in np.asarray(P, np.float32).ravel()) + "]\n")


def scene_text(light, meshes, material='Material "matte" "color Kd" [.6 .6 .6]\n', xres=64, yres=64, spp=4, maxdepth=3, extra=""):
    body = 'LightSource "point" "point from" [%.9g %.9g %.9g] "color I" [20 20 20]\n' % tuple(light) + material
    return HEAD % (xres, yres, spp, maxdepth) + body + "".join(mesh(P, idx) for P, idx in meshes) + extra + "WorldEnd\n"


def text_triangles(text):
    """[n, 9] float32 triangles of every trianglemesh of `text`, in creation order (the meshes carry no transform)"""
    out = []
    for m in re.finditer(r'"integer indices" \[([^\]]*)\] "point P" \[([^\]]*)\]', text):
        idx = np.array(m.group(1).split(), np.int64).reshape(-1, 3)
        P = np.array(m.group(2).split(), np.float64).astype(np.float32).reshape(-1, 3)
        out.append(P[idx].reshape(-1, 9))
    return np.concatenate(out).astype(np.float32)


def text_light(text):
    m = re.search(r'"point from" \[([^\]]*)\]', text)
    return np.array(m.group(1).split(), np.float64).astype(np.float32)


def soup(n, seed, centre_lo=-3.0, centre_hi=3.0, size=0.25):
    rng = np.random.default_rng(seed)
    c = rng.uniform(centre_lo, centre_hi, (n, 1, 3))
    P = (c + rng.normal(scale=size, size=(n, 3, 3))).astype(np.float32).reshape(-1, 3)
    return P, np.arange(3 * n).reshape(-1, 3)


def floor(z=-3.5, half=5.0):
    return np.array([[-half, -half, z], [half, -half, z], [half, half, z], [-half, half, z]], np.float32), np.array([[0, 1, 2], [0, 2, 3]])


# name -> (text, near list: "empty" | "some")
def scenes():
    atrium = scene_gen.atrium(0.1, xres=64, yres=64, spp=16, maxdepth=5)[0]
    L0 = np.array([0.125, 0.25, 0.375], np.float32)      # (dyadic: light - v is exact for the short v of the boundary rays)
    sp = soup(2000, 1)
    # one triangle 1e-4 from the light, one degenerate (two equal vertices) and one with collinear vertices, among a small soup
    nearP = np.array([[0.125, 0.25, 0.375 - 1e-4], [0.625, 0.25, 0.375 - 1e-4], [0.125, 0.75, 0.375 - 1e-4],
                      [1, 1, 1], [1, 1, 1], [1.5, 1, 1.2],
                      [-1, -1, 0], [-1.5, -1.5, 0.5], [-2, -2, 1]], np.float32)
    s2 = soup(300, 2)
    outside = soup(500, 3, centre_lo=-2.0, centre_hi=2.0)
    # the light in the plane of a large triangle (z = 0.375 exactly) that does not contain it, and on the line of one edge of another
    planeP = np.array([[1, -4, 0.375], [5, -4, 0.375], [3, 5, 0.375], [0.125, 1.0, 0.375], [0.125, 2.0, 0.375], [1.0, 2.0, 0.9]], np.float32)
    s4 = soup(300, 4)
    return {
        "atrium": (atrium, "empty"),
        "soup": (scene_text(L0, [sp, floor()]), "empty"),
        "near": (scene_text(L0, [(nearP, np.arange(9).reshape(3, 3)), s2, floor()]), "some"),
        "outside": (scene_text(np.array([9.0, -7.5, 6.0], np.float32), [outside, floor()]), "empty"),
        "inplane": (scene_text(L0, [(planeP, np.arange(6).reshape(2, 3)), s4, floor()]), "empty"),
    }


def grid_scene(hprt, model, res=None, grid="1"):
    """Scene(model) on device 0 created under HPRT_SHADOW_GRID_RES = res (None: the default) and HPRT_SHADOW_GRID = grid — "1" a grid
    whatever its lists' lengths, "0" none, None the default (a grid only where it is expected to beat the walk)"""
    env = {"HPRT_SHADOW_GRID_RES": None if res is None else str(res), "HPRT_SHADOW_GRID": grid}
    old = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
        return hprt.Scene(model, hprt.Bvh(model), device=0)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def cell_of(d, R):
    """The device's sg_cell (csrc/device/shadow_grid.hip) of the directions -d, [n, 3] float32, restated operation for operation:
    (cell, su, sv) — the cell and the sixteenth of it along u and v"""
    d = np.asarray(d, np.float32)
    x, y, z = -d[:, 0], -d[:, 1], -d[:, 2]
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    a0 = (ax >= ay) & (ax >= az)
    a1 = ~a0 & (ay >= az)
    mj = np.where(a0, x, np.where(a1, y, z)); a = np.where(a0, y, np.where(a1, z, x)); b = np.where(a0, z, np.where(a1, x, y))
    m = np.abs(mj)
    with np.errstate(all="ignore"):
        u = (a / m).astype(np.float32); v = (b / m).astype(np.float32)
        scale = np.float32(8.0 * R)
        fu = np.floor(((u + np.float32(1)) * scale).astype(np.float32)); fv = np.floor(((v + np.float32(1)) * scale).astype(np.float32))
    fu = np.clip(np.nan_to_num(fu, nan=0.0, posinf=16 * R, neginf=-1), 0, 16 * R - 1).astype(np.int64)
    fv = np.clip(np.nan_to_num(fv, nan=0.0, posinf=16 * R, neginf=-1), 0, 16 * R - 1).astype(np.int64)
    face = np.where(a0, 0, np.where(a1, 2, 4)) + (mj < 0)
    return (face * R + (fv >> 4)) * R + (fu >> 4), fu & 15, fv & 15


def triangle_points():
    """64 barycentric weights: the vertices, points along the edges, interior points"""
    w = [(1, 0, 0), (0, 1, 0), (0, 0, 1)]
    for t in (0.5, 0.25, 0.75, 1e-3, 1 - 1e-3, 0.1, 0.9):
        w += [(1 - t, t, 0), (0, 1 - t, t), (t, 0, 1 - t)]
    rng = np.random.default_rng(7)
    while len(w) < 64:
        a, b = rng.random(2)
        if a + b > 1:
            a, b = 1 - a, 1 - b
        w.append((1 - a - b, a, b))
    return np.array(w, np.float64)
