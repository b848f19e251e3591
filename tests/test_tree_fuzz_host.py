"""The input conditions of the tree fuzz (tests/tree_fuzz.py), on the CPU: every committed (config, seed) pair is a usable input
for tests/test_gpu_tree_fuzz.py — conditions on the scenes, the trees and the references, none of them a measurement of a device
walk.  The scene parses without warnings; a film seed's scene has primitives and lights and the oracle's render of it is not
black and traces shadow rays; the library builds the tree, within five seconds (and through two-level trees a ray with a
NaN direction stays under 200,000 nodes: past that the device test takes minutes); on 20,000 camera rays and
20,000 random rays the restated walk over that tree finds the oracle's closest hit on a film seed — primitive, instance, the bits of t and of the
barycentrics, so the film through the tree is the oracle's — and on a tie seed the oracle's t on every ray but another of the
coincident surfaces on at least a hundred.  Each config's film seeds together reach spheres, area and infinite lights, image
textures, paths of several bounces and (two-level) mirrored instances; all configs together every material kind.  And the
generator in default mode still writes the scenes tests/test_gpu_fuzz.py was written for."""
import hashlib
import time

import numpy as np
import pytest

import tree_fuzz as tf
from test_gpu_fuzz import random_scene
from tree_walk_checks import _bits

MAX_BUILD_SECONDS = 5.0
MAX_NAN_RAY_NODES = 200000      # two-level walks: the nodes a ray with a NaN direction visits (it enters every object tree it meets)
_scenes, _pairs = {}, {}


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("tree_fuzz")


def _scene(hprt, orc, d, objects, seed, tie):
    """a generated scene, once for all the configs that use it: its traits, the oracle's render (film seeds), the probe rays and
    the oracle's hits on them"""
    key = (objects, seed, tie)
    if key not in _scenes:
        text = random_scene(seed, objects=objects, twins=tie)
        m, path = tf.bake(hprt, d, text, "o%d_s%d_%s" % (objects, seed, "tie" if tie else "film"))
        oracle = orc.OracleScene(path)
        s = {"model": m, "path": path, "traits": tf.traits(text, m)}
        if not tie:
            _, film, c0, _, _ = oracle.render(threads=8)
            s["film_max"], s["shadow_rays"] = float(film[..., :3].max()), c0["shadow_rays"]
        s["rays"] = tf.joined(tf.probe_rays(m, oracle, hprt.Bvh(m).info()["bounds"], seed))
        s["hits"] = oracle.intersect_inst(*s["rays"])[:4]
        _scenes[key] = s
    return _scenes[key]


def _pair(hprt, orc, d, name, seed, tie):
    """the scene of a pair, the seconds the library's build took and the restated walk's hits on the probe rays"""
    key = (name, seed, tie)
    if key not in _pairs:
        c = tf.CONFIGS[name]
        s = _scene(hprt, orc, d, c.objects, seed, tie)
        t = time.perf_counter()
        tree = c.make(hprt, s["model"])          # (an HprtError here is a refused tree: the pair is no input)
        seconds = time.perf_counter() - t
        ref = c.restate(s["path"], tree)
        _pairs[key] = (s, seconds, c.closest(ref, *s["rays"]))
        if c.two_level:
            o = np.array([[0.3, 0.2, 0.1]], np.float32)
            nodes = int(ref.intersect(o, np.full((1, 3), np.nan, np.float32), np.full(1, np.inf, np.float32))[4][0, 0])
            assert nodes <= MAX_NAN_RAY_NODES, (name, seed, nodes)
    return _pairs[key]


def test_the_lists_are_complete():
    assert list(tf.CONFIGS) == ["kd", "rbsp7", "rbsp13", "rbspkd9", "bsppaper", "bsppaperkd", "bsprandomfastkd", "bspclusterwithkd", "kdinst",
                                "rbspinst13", "rbspkdinst9"]
    for c in tf.CONFIGS.values():
        assert len(set(c.film)) == 4 and len(set(c.ties)) == 2, c.name
        # (0-63, but for the two-level walks' second tie seed: tests/tree_fuzz.py says why)
        assert all(0 <= s < 64 for s in c.film + c.ties if not (c.two_level and s == c.ties[1] == 122)), c.name


@pytest.mark.parametrize("name,seed", tf.FILM_PAIRS, ids=["%s-%d" % p for p in tf.FILM_PAIRS])
def test_film_pair_is_an_input(hprt, orc, workdir, name, seed):
    s, seconds, (t1, p1, i1, b1) = _pair(hprt, orc, workdir, name, seed, False)
    tr = s["traits"]
    assert tr["primitives"] > 0 and tr["lights"] >= 1, tr
    assert s["film_max"] > 0 and s["shadow_rays"] > 0, (s["film_max"], s["shadow_rays"])
    assert seconds <= MAX_BUILD_SECONDS, seconds
    t0, p0, i0, b0 = s["hits"]
    assert np.array_equal(p0, p1) and np.array_equal(i0, i1), (int((p0 != p1).sum()), int((i0 != i1).sum()))
    assert np.array_equal(_bits(t0), _bits(t1)) and np.array_equal(_bits(b0), _bits(b1))
    assert (p0 >= 0).sum() > 1000      # (the probe rays do reach the scene)


@pytest.mark.parametrize("name,seed", tf.TIE_PAIRS, ids=["%s-%d" % p for p in tf.TIE_PAIRS])
def test_tie_pair_is_an_input(hprt, orc, workdir, name, seed):
    s, seconds, (t1, p1, i1, b1) = _pair(hprt, orc, workdir, name, seed, True)
    assert s["traits"]["primitives"] > 0 and seconds <= MAX_BUILD_SECONDS, (s["traits"], seconds)
    t0, p0, i0, b0 = s["hits"]
    assert np.array_equal(_bits(t0), _bits(t1))
    assert ((p0 != p1) | (i0 != i1)).sum() >= 100, int(((p0 != p1) | (i0 != i1)).sum())


@pytest.mark.parametrize("name", list(tf.CONFIGS))
def test_a_configs_film_seeds_reach_what_the_bvh_fuzz_reaches(hprt, orc, workdir, name):
    c = tf.CONFIGS[name]
    scenes = [_scene(hprt, orc, workdir, c.objects, seed, False) for seed in c.film]
    tr = [s["traits"] for s in scenes]
    assert sum(t["sphere"] for t in tr) >= 2          # the QUAD variants of the walk
    assert any(t["area"] for t in tr) and any(t["infinite"] for t in tr) and any(t["textures"] for t in tr)
    assert sum(t["maxdepth"] >= 2 for t in tr) >= 3
    if c.two_level:
        assert all((s["hits"][2] >= 0).sum() >= 1000 for s in scenes), [int((s["hits"][2] >= 0).sum()) for s in scenes]
        assert any(t["mirrored"] for t in tr)


def test_all_configs_together_reach_every_material_kind(hprt, orc, workdir):
    kinds = set()
    for c in tf.CONFIGS.values():
        for seed in c.film:
            kinds |= _scene(hprt, orc, workdir, c.objects, seed, False)["traits"]["materials"]
    assert kinds == set(tf.MATERIAL_KINDS), sorted(set(tf.MATERIAL_KINDS) - kinds)


def test_the_default_generator_is_unchanged():
    """random_scene(seed) writes, for seeds 0-63, the text it wrote before it had its two switches: tests/test_gpu_fuzz.py's
    scenes are the same scenes"""
    h = hashlib.sha256("\x00".join(random_scene(seed) for seed in range(64)).encode()).hexdigest()
    assert h == DEFAULT_TEXT_SHA256


DEFAULT_TEXT_SHA256 = "ca81f6d9fa6d325dda6be1d64a05cb4621c237337167a9c1fa9d894af79fdc48"
