"""The input conditions of the tree fuzz for the two-level general BSP walks (tests/bsppaperinst_fuzz.py), on the CPU — what
tests/test_tree_fuzz_host.py asserts for the eleven other configs, restated here because its helpers look a config up
in tree_fuzz.CONFIGS: every committed (config, seed) pair is a usable input for tests/test_gpu_bsppaperinst_fuzz.py.  The scene parses
without warnings; a film seed's scene has primitives and lights and the oracle's render of it is not black and traces shadow rays;
the library builds the trees within five seconds; a ray with a NaN direction stays under 200,000 nodes; on 20,000 camera rays and
20,000 random rays the restated walk over the library's trees finds the oracle's closest hit on a film seed — primitive, instance,
the bits of t and of the barycentrics — and on a tie seed the oracle's t on every ray but another of the coincident surfaces on at
least a hundred.  Each config's film seeds reach spheres, area and infinite lights, image textures, paths of several bounces, a
thousand probe hits inside instances and a mirrored instance.  None of it measures a device walk."""
import time

import numpy as np
import pytest

import bsppaperinst_fuzz as bf
import tree_fuzz as tf
from test_gpu_fuzz import random_scene
from tree_walk_checks import _bits

MAX_BUILD_SECONDS = 5.0
MAX_NAN_RAY_NODES = 200000      # the nodes a ray with a NaN direction visits (it enters every object tree it meets)
_scenes, _pairs = {}, {}


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("bsppaperinst_fuzz")


def _scene(hprt, orc, d, objects, seed, tie):
    """a generated scene, once for both configs: its traits, the oracle's render (film seeds), the probe rays and the oracle's hits"""
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
    """the scene of a pair, the seconds the library's build took, the restated walk's hits on the probe rays and the nodes of a NaN ray"""
    key = (name, seed, tie)
    if key not in _pairs:
        c = bf.CONFIGS[name]
        s = _scene(hprt, orc, d, c.objects, seed, tie)
        t = time.perf_counter()
        tree = c.make(hprt, s["model"])          # (an HprtError here is a refused tree: the pair is no input)
        seconds = time.perf_counter() - t
        ref = c.restate(s["path"], tree)
        o = np.array([[0.3, 0.2, 0.1]], np.float32)
        nodes = int(ref.intersect(o, np.full((1, 3), np.nan, np.float32), np.full(1, np.inf, np.float32))[4][0, 0])
        _pairs[key] = (s, seconds, c.closest(ref, *s["rays"]), nodes)
    return _pairs[key]


def test_the_lists_are_complete():
    assert list(bf.CONFIGS) == ["bsppaperinst", "bsppaperkdinst"]
    assert not set(bf.CONFIGS) & set(tf.CONFIGS)
    for c in bf.CONFIGS.values():
        assert c.two_level and c.objects == 2 and c.attach == "attach_bsppaperinst"
        assert len(set(c.film)) >= 4 and len(set(c.ties)) >= 2, c.name
    assert bf.CONFIGS["bsppaperkdinst"].kd_aware and not bf.CONFIGS["bsppaperinst"].kd_aware


@pytest.mark.parametrize("name,seed", bf.FILM_PAIRS, ids=["%s-%d" % p for p in bf.FILM_PAIRS])
def test_film_pair_is_an_input(hprt, orc, workdir, name, seed):
    s, seconds, (t1, p1, i1, b1), nan_nodes = _pair(hprt, orc, workdir, name, seed, False)
    tr = s["traits"]
    assert tr["primitives"] > 0 and tr["lights"] >= 1, tr
    assert s["film_max"] > 0 and s["shadow_rays"] > 0, (s["film_max"], s["shadow_rays"])
    assert seconds <= MAX_BUILD_SECONDS, seconds
    assert nan_nodes <= MAX_NAN_RAY_NODES, nan_nodes
    t0, p0, i0, b0 = s["hits"]
    assert np.array_equal(p0, p1) and np.array_equal(i0, i1), (int((p0 != p1).sum()), int((i0 != i1).sum()))
    assert np.array_equal(_bits(t0), _bits(t1)) and np.array_equal(_bits(b0), _bits(b1))
    assert (p0 >= 0).sum() > 1000      # (the probe rays do reach the scene)


@pytest.mark.parametrize("name,seed", bf.TIE_PAIRS, ids=["%s-%d" % p for p in bf.TIE_PAIRS])
def test_tie_pair_is_an_input(hprt, orc, workdir, name, seed):
    s, seconds, (t1, p1, i1, b1), nan_nodes = _pair(hprt, orc, workdir, name, seed, True)
    assert s["traits"]["primitives"] > 0 and seconds <= MAX_BUILD_SECONDS, (s["traits"], seconds)
    assert nan_nodes <= MAX_NAN_RAY_NODES, nan_nodes
    t0, p0, i0, b0 = s["hits"]
    assert np.array_equal(_bits(t0), _bits(t1))
    assert ((p0 != p1) | (i0 != i1)).sum() >= 100, int(((p0 != p1) | (i0 != i1)).sum())


@pytest.mark.parametrize("name", list(bf.CONFIGS))
def test_a_configs_film_seeds_reach_what_the_bvh_fuzz_reaches(hprt, orc, workdir, name):
    c = bf.CONFIGS[name]
    scenes = [_scene(hprt, orc, workdir, c.objects, seed, False) for seed in c.film]
    tr = [s["traits"] for s in scenes]
    assert sum(t["sphere"] for t in tr) >= 2          # the QUAD variants of the walk
    assert any(t["area"] for t in tr) and any(t["infinite"] for t in tr) and any(t["textures"] for t in tr)
    assert sum(t["maxdepth"] >= 2 for t in tr) >= 3
    assert all((s["hits"][2] >= 0).sum() >= 1000 for s in scenes), [int((s["hits"][2] >= 0).sum()) for s in scenes]
    assert any(t["mirrored"] for t in tr)
