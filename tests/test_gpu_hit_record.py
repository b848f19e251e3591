"""The closest-hit record (device/kernels.h, HitStream): one 16-byte word {b0, b1, b2, primitive word} per ray, stored once per accepted
hit, and a second word {t, instance} that exists only for the callers that read it — the ray-call entry points (t) and scenes with
object instances (the instance).  Held here: the ray calls still return the oracle's t, primitive, instance and barycentrics bit for
bit from both walks, on ray sets that hold misses and rays whose first accepted hit is replaced by a closer one; a render of a scene
without instances reads nothing of the planes it no longer has; the instance still reaches k_shade; the MIS ray's hit still reaches
k_resolve, from the BVH walk and from an attached tree's."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, KILLEROO, ROOT
from tree_walk_checks import _srgb8

pytestmark = pytest.mark.gpu

FIXTURES = {"killeroo": os.path.join(GOLDEN, "killeroo.hprt"),                    # triangles only
            "killeroo-simple": KILLEROO,                                           # triangles and the quadric emitter
            "simple-instanced": os.path.join(GOLDEN, "simple_instanced.hprt")}    # eight spheres in one object instance
N_RAYS = 4096
CROP = (0.42, 0.42 + 64 / 700.0, 0.47, 0.47 + 64 / 700.0)      # 64 x 64 pixels of killeroo-simple: killeroo, floor and the light's highlight
SPP = 4


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _visit_rank(oracle):
    """rank[octant][primitive] and aggregate[primitive]: the position of every ordered primitive (numbered as hprt_intersect_instanced
    numbers them: top level, then object 0, 1, ...) in the order in which BVHAccel::Intersect comes to the primitives of its aggregate
    for a ray of that direction octant (bit a of the octant: d[a] < 0).  The walk (accelerators/bvh.cpp:358-399) is a depth-first
    descent that takes the second child first where the ray is negative along the node's split axis; what it skips because of the hits
    it already holds only drops out of that order, and a leaf's primitives are tested in storage order.  Both device walks keep the
    reference's order for closest-hit rays."""
    ranks, aggregate = [[] for _ in range(8)], []
    for a, (nodes, order) in enumerate([oracle.bvh_arrays()] + oracle.object_bvh_arrays()):
        n_prims = order.shape[0]
        aggregate.append(np.full(n_prims, a, np.int64))
        axis = (nodes[:, 7] & 3).tolist(); count = (nodes[:, 7] >> 2).tolist(); offset = nodes[:, 6].tolist()      # axis 3: a leaf
        for octant in range(8):
            rank = np.zeros(n_prims, np.int64)
            stack, seen = [0] if nodes.shape[0] else [], 0
            while stack:
                k = stack.pop()
                if axis[k] == 3:
                    rank[offset[k]:offset[k] + count[k]] = np.arange(seen, seen + count[k]); seen += count[k]
                elif (octant >> axis[k]) & 1: stack.append(k + 1); stack.append(offset[k])      # (popped last = visited later)
                else: stack.append(offset[k]); stack.append(k + 1)
            assert seen == n_prims
            ranks[octant].append(rank)
    return np.stack([np.concatenate(r) for r in ranks]), np.concatenate(aggregate)


def _replaced(oracle, order, o, d, tmax):
    """(replaced, missed) per ray, from the oracle's hit list — the closest hit N and the next three hits behind it, each found by the
    oracle from just behind the one before.  A ray REPLACES its first accepted hit if some farther hit F of the list lies in N's
    aggregate and comes before N in the walk's order: F's leaf and every box above it are pierced in front of the ray's tMax, so when
    the walk gets there it either accepts F or has already accepted something that hides it, and N, tested later, overwrites that
    record.  (Instances: the fixture's one instance has the identity transform, so the instance-space ray has the world ray's octant.
    A surface inside the 1e-4 sliver behind a hit is not listed: that can hide a case, it cannot fake one.)"""
    rank, aggregate = order
    octant = ((d[:, 0] < 0) * 1 + (d[:, 1] < 0) * 2 + (d[:, 2] < 0) * 4).astype(np.int64)
    t1, p1, _, _, _ = oracle.intersect_inst(o, d, tmax)
    hit = p1 >= 0
    replaced = np.zeros(o.shape[0], bool)
    oc, left, alive = o.copy(), tmax.copy(), hit.copy()
    t, p = t1, p1
    for _ in range(3):
        step = np.where(alive, t * np.float32(1.0001) + np.float32(1e-6), np.float32(0)).astype(np.float32)
        oc = (oc + d * step[:, None]).astype(np.float32)
        left = np.where(alive, left - step, np.float32(0)).astype(np.float32)
        t, p, _, _, _ = oracle.intersect_inst(oc, d, left)
        alive = alive & (p >= 0)
        k = np.nonzero(alive & (p != p1))[0]
        replaced[k] |= (aggregate[p[k]] == aggregate[p1[k]]) & (rank[octant[k], p[k]] < rank[octant[k], p1[k]])
    return replaced & np.all(d != 0, axis=1), ~hit


def _ray_set(oracle, seed):
    """4,096 rays: a quarter through and past the scene at random, the rest aimed ALONG rows of primitives — chords from in front of
    one surface point of the scene through a neighbouring one, which graze the surface and pierce several primitives in a row — with a
    preference for those the hit list proves to replace a hit."""
    rng = np.random.default_rng(seed)
    order = _visit_rank(oracle)
    b = np.array(oracle.bvh_info()["bounds"], np.float32)
    lo, hi = b[:3], b[3:]
    centre, radius = (lo + hi) * np.float32(0.5), np.float32(0.5 * np.linalg.norm(hi - lo))

    def through_the_scene(n, spread):
        v = rng.normal(size=(n, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
        o = (centre + v * radius * 1.5).astype(np.float32)
        target = centre + rng.uniform(-spread, spread, (n, 3)) * (hi - lo)
        return o, (target - o).astype(np.float32), np.full(n, np.inf, np.float32)

    # surface points, sorted along the scene's longest axis: neighbours in that order are close together on the surface
    so, sd, stm = through_the_scene(40000, 0.5)
    t, p, _, _, _ = oracle.intersect_inst(so, sd, stm)
    X = (so[p >= 0] + sd[p >= 0] * t[p >= 0, None]).astype(np.float32)
    X = X[np.argsort(X[:, int(np.argmax(hi - lo))])]
    far, near = X[:-1:2], X[1::2]
    far, near = np.concatenate([far, near]), np.concatenate([near, far])      # (every chord in both directions)
    chord = (far - near).astype(np.float32)
    co = (near - chord * np.float32(0.5)).astype(np.float32)
    ctm = np.full(co.shape[0], np.inf, np.float32)
    ctm[::3] = np.float32(4.0)                     # (a third as segments that end behind the far point)
    good, _ = _replaced(oracle, order, co, chord, ctm)
    pick = np.nonzero(good)[0]
    pick = pick[rng.permutation(pick.shape[0])[:N_RAYS // 2]]
    rest = np.setdiff1d(np.arange(co.shape[0]), pick)
    rest = rest[rng.permutation(rest.shape[0])[:N_RAYS // 4]]
    n_random = N_RAYS - pick.shape[0] - rest.shape[0]
    ro, rd, rtm = through_the_scene(n_random, 0.9)      # (wide of the scene: many of these miss)
    o = np.concatenate([co[pick], co[rest], ro]); d = np.concatenate([chord[pick], chord[rest], rd]).astype(np.float32)
    tmax = np.concatenate([ctm[pick], ctm[rest], rtm])
    mix = rng.permutation(N_RAYS)                   # the kinds mixed within every wavefront
    return np.ascontiguousarray(o[mix]), np.ascontiguousarray(d[mix]), np.ascontiguousarray(tmax[mix]), order


_BINARY_WALK_CHILD = r"""
import importlib, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
hprt = importlib.import_module("thesis-pbrt-v3_amd")
r = np.load(sys.argv[3])
m = hprt.Model.load(sys.argv[2])
sc = hprt.Scene(m, hprt.Bvh(m), device=0)
t, p, i, b = sc.intersect_instanced(r["o"], r["d"], r["tmax"])
np.savez(sys.argv[4], t=t, p=p, i=i, b=b)
"""


@pytest.mark.parametrize("name", list(FIXTURES))
def test_ray_calls_return_the_same_hits_from_both_walks(hprt, orc, tmp_path, name):
    path = FIXTURES[name]
    oracle = orc.OracleScene(path)
    o, d, tmax, order = _ray_set(oracle, 11)
    assert o.shape == (N_RAYS, 3)
    replaced, missed = _replaced(oracle, order, o, d, tmax)
    print("%s: %d rays, %d miss, %d replace their first accepted hit" % (name, N_RAYS, int(missed.sum()), int(replaced.sum())))
    assert missed.sum() >= 100 and replaced.sum() >= 100, (int(missed.sum()), int(replaced.sum()))
    t0, p0, i0, b0, _ = oracle.intersect_inst(o, d, tmax)
    # the wide walk (k_walk4), in this process
    m = hprt.Model.load(path)
    sc = hprt.Scene(m, hprt.Bvh(m), device=0)
    t1, p1, i1, b1 = sc.intersect_instanced(o, d, tmax)
    # the binary walk (k_trace): HPRT_WIDE_WALK is read once per process, so a fresh child traces the same rays
    np.savez(tmp_path / "rays.npz", o=o, d=d, tmax=tmax)
    env = dict(os.environ, HPRT_WIDE_WALK="0")
    subprocess.run([sys.executable, "-c", _BINARY_WALK_CHILD, ROOT, path, str(tmp_path / "rays.npz"), str(tmp_path / "hits.npz")],
                   env=env, check=True, timeout=120)
    h = np.load(tmp_path / "hits.npz")
    t2, p2, i2, b2 = h["t"], h["p"], h["i"], h["b"]
    for what, (t, p, i, b) in (("wide", (t1, p1, i1, b1)), ("binary", (t2, p2, i2, b2))):
        assert np.array_equal(p0, p), (what, int((p0 != p).sum()))
        assert np.array_equal(i0, i), (what, int((i0 != i).sum()))
        assert np.array_equal(_bits(t0), _bits(t)), what
        assert np.array_equal(_bits(b0), _bits(b)), what
    assert np.array_equal(p1, p2) and np.array_equal(i1, i2) and np.array_equal(_bits(t1), _bits(t2)) and np.array_equal(_bits(b1), _bits(b2))
    if name == "simple-instanced":
        assert (i0[p0 >= 0] >= 0).any()


def _crop_options(model, crop, spp):
    opt = model.options.copy()
    for k in range(4):
        opt.crop[k] = crop[k]
    opt.spp = spp
    return opt


@pytest.fixture(scope="module")
def killeroo_crop_film(killeroo_oracle):
    """the oracle's film of the 64 x 64 crop at 4 spp, computed once for the tests below"""
    killeroo_oracle.set_film(crop=CROP, spp=SPP)
    _, film, _, _, _ = killeroo_oracle.render(spp=SPP, threads=8)
    killeroo_oracle.set_film(crop=(0, 1, 0, 1), spp=8)
    film.setflags(write=False)
    return film


def test_render_without_instances_reads_no_second_hit_word(killeroo_model, killeroo_scene, killeroo_crop_film):
    """A scene without object instances has no hit.b / misHit.b planes.  With every scratch byte 0xFF before the render — a hit word
    of all ones is a miss, a float of all ones a NaN — the film is the un-poisoned one: every record that is read was written in full
    (misses included), and nothing reads a plane that is not there."""
    opt = _crop_options(killeroo_model, CROP, SPP)
    film, _ = killeroo_scene.render(opt)
    assert np.array_equal(_bits(film), _bits(killeroo_crop_film))
    try:
        killeroo_scene.debug_poison(0xFF)
        poisoned, _ = killeroo_scene.render(opt)
        poisoned_all, _ = killeroo_scene.render(opt, trace_all=True)
    finally:
        killeroo_scene.debug_poison(None)
    assert np.array_equal(_bits(poisoned), _bits(film))
    assert np.array_equal(_bits(poisoned_all), _bits(film))
    assert float(film[..., :3].max()) > 0


def test_instanced_render_still_carries_the_instance_to_shading(hprt, orc):
    path = FIXTURES["simple-instanced"]
    m = hprt.Model.load(path)
    sc = hprt.Scene(m, hprt.Bvh(m), device=0)
    crop = (0.40, 0.40 + 64 / 700.0, 0.40, 0.40 + 64 / 700.0)
    opt = _crop_options(m, crop, SPP)
    oracle = orc.OracleScene(path)
    oracle.set_film(crop=crop, spp=SPP)
    _, film0, _, _, _ = oracle.render(spp=SPP, threads=8)
    try:
        sc.debug_poison(0xFF)
        film1, _ = sc.render(opt)
    finally:
        sc.debug_poison(None)
    assert np.array_equal(_bits(film0), _bits(film1)), int(np.any(film0 != film1, axis=2).sum())
    assert float(film0[..., :3].max()) > 0      # (the spheres are in the crop: every lit pixel went through the instance transform)


def test_mis_ray_hits_reach_the_resolve_pass(hprt, killeroo_model, killeroo_scene, killeroo_crop_film):
    """killeroo-simple's area light is sampled with an MIS ray whose closest hit (VertexStreams::misHit) k_resolve reads: word and
    barycentrics.  trace_all traces every such ray.  From the BVH walk the film is the oracle's bit for bit.  From an attached kd-tree
    (the walk of kd_walk.hip writes the records) a tie in t between two touching triangles may fall the other way, so a few samples
    take another path: that film is held to the oracle's as tests/tree_walk_checks.py holds the kd-tree's films of this scene to the
    reference's image — 8-bit sRGB, mean difference below 0.002 levels, none above 9, above 2 in fewer than 3e-4 of the pixels.  A
    wrong word or barycentric in misHit would move every pixel the light reaches through an MIS ray."""
    opt = _crop_options(killeroo_model, CROP, SPP)
    film_all, st_all = killeroo_scene.render(opt, trace_all=True)
    _, st = killeroo_scene.render(opt)
    assert st_all["rays"] > st["rays"]      # (the MIS rays a plain render proves useless are traced here)
    assert np.array_equal(_bits(film_all), _bits(killeroo_crop_film))
    sc = hprt.Scene(killeroo_model, hprt.Bvh(killeroo_model), device=0)
    sc.attach_kdtree(hprt.KdTree(killeroo_model))
    ref = _srgb8(hprt.film_resolve(np.array(killeroo_crop_film), opt.film_scale))
    for trace_all in (False, True):
        walked, _ = sc.render(opt, trace_all=trace_all)
        rgb = hprt.film_resolve(walked, opt.film_scale)
        d = np.abs(_srgb8(rgb) - ref).astype(np.float64)
        print("kdtree render, trace_all=%s: sRGB8 mean |d| %g, max %g, share above 2: %g, %d pixels differ"
              % (trace_all, d.mean(), d.max(), (d > 2).mean(), int((d.max(axis=2) > 0).sum())))
        assert np.isfinite(rgb).all() and float(rgb.max()) > 0
        assert d.mean() < 0.002 and d.max() <= 9 and (d > 2).mean() < 3e-4, (d.mean(), d.max(), (d > 2).mean())
