"""What the tree fuzz shares (tests/test_tree_fuzz_host.py on the CPU, tests/test_gpu_tree_fuzz.py on the GPU): the random scenes
of tests/test_gpu_fuzz.py rendered through every tree walk instead of the BVH.  CONFIGS names the walks — how each one's tree is
built from a model (keyword parameters: a generated scene has no Accelerator line), attached to a scene and restated on the CPU —
and the committed (config, seed) lists: four FILM seeds whose scene has no ties (random_scene(seed, objects, twins=False)), so
that the walk finds the oracle's hit on every ray and the film through the tree is the oracle's film bit for bit, and two TIE
seeds (twins=True) on which the tree's traversal order settles coincident surfaces differently from the BVH's.  The single-level
walks take the scenes without objects (objects=0), the two-level ones those with two (objects=2).

The seeds were picked from 0-63 by the conditions tests/test_tree_fuzz_host.py asserts; none of them is a
measurement of the code under test.  One seed lies beyond 63, the two-level walks' second tie seed 122: of 0-63 only 31 and 59
meet the tie conditions with trees that build in five seconds, and on 31 a ray with a NaN direction, to which every comparison
is false, walks every object tree under every top-level leaf that holds its instance: millions of nodes in the restatement,
minutes in a lane of the device walk.  The two-level seeds are those whose scene such a ray crosses in under 200,000 nodes.  Every restatement walks the LIBRARY's tree (set_tree / take): the restated builds are held
to the library's elsewhere (tests/test_*_host.py) and are slow on a thousand primitives.  A node-based tree is a tree over
BSPNode (plain, withkd) or BSPKdNode (fastkd), restated by the scene types tests/bspnode_reference.cpp itself walks with:
bsppaper's and bsppaperkd's."""
import re

import numpy as np

import bsppaperkd_ref
import kdinst_ref
import rbspinst_ref
import tree_ref
import tree_walk_checks as twc
from test_gpu_fuzz import random_scene
from test_gpu_textures import _write_images

N_PROBE = 20000          # camera rays and as many random rays per scene on the CPU
N_PROBE_GPU = 4096       # the first so many of each family on the GPU
NODE_K, NODE_SEED = 5, 7
MATERIAL_KINDS = ("matte", "oren", "plastic", "mirror", "glass", "metal", "substrate", "uber", "textured")      # _material's


class Config:
    """One tree walk: make(hprt, model) builds its tree, attach names the Scene method, restate(path, tree) gives the restatement
    over the library's arrays.  two_level: a walk of instanced scenes (intersect returns the instance too); kd_aware: a fifth
    (two-level: sixth) counter column, Scene.kd_counters() and pixel_kd_stats()."""

    def __init__(self, name, make, attach, restate, film, ties, two_level=False, kd_aware=False):
        self.name, self.make, self.attach, self.restate = name, make, attach, restate
        self.film, self.ties, self.two_level, self.kd_aware = tuple(film), tuple(ties), two_level, kd_aware
        self.objects = 2 if two_level else 0

    def text(self, seed, tie=False):
        return random_scene(seed, objects=self.objects, twins=tie)

    def closest(self, ref, o, d, tm):
        """(t, primitive, instance, barycentrics) of the restated walk; a single-level walk has no instances"""
        r = ref.intersect(o, d, tm)
        if self.two_level:
            return r[0], r[1], r[2], r[3]
        return r[0], r[1], np.full(r[1].shape[0], -1, np.int32), r[2]


def _set(scene, tree):
    scene.set_tree(*tree.arrays()[:2])
    return scene


def _node(acc):
    return lambda hprt, m: hprt.bspnode_tree(m, acc, n_directions=NODE_K, seed=NODE_SEED)[0]


# (the single-level configs share their seeds where the conditions allow it, the two-level ones too: a scene is parsed and
# rendered by the oracle once for all of them)
CONFIGS = {c.name: c for c in [
    Config("kd", lambda hprt, m: hprt.KdTree(m), "attach_kdtree",
           lambda path, tree: _set(tree_ref.KdScene(path), tree), film=(36, 15, 24, 12), ties=(5, 59)),
    Config("rbsp7", lambda hprt, m: hprt.Rbsp(m, n_directions=7), "attach_rbsp",
           lambda path, tree: _set(tree_ref.RbspScene(path, 7, build=False), tree), film=(11, 34, 23, 57), ties=(5, 12)),
    Config("rbsp13", lambda hprt, m: hprt.Rbsp(m, n_directions=13), "attach_rbsp",
           lambda path, tree: _set(tree_ref.RbspScene(path, 13, build=False), tree), film=(21, 30, 42, 1), ties=(12, 37)),
    Config("rbspkd9", lambda hprt, m: hprt.RbspKd(m, n_directions=9), "attach_rbspkd",
           lambda path, tree: _set(tree_ref.RbspKdScene(path, 9, build=False), tree), film=(36, 15, 24, 12), ties=(5, 59), kd_aware=True),
    Config("bsppaper", lambda hprt, m: hprt.BspPaper(m, isect_cost=80), "attach_bsppaper",
           lambda path, tree: _set(tree_ref.BspScene(path, build=False), tree), film=(21, 30, 42, 1), ties=(12, 19)),
    Config("bsppaperkd", lambda hprt, m: hprt.BspPaperKd(m, isect_cost=80), "attach_bsppaperkd",
           lambda path, tree: _set(bsppaperkd_ref.BspKdScene(path, build=False), tree), film=(11, 34, 23, 57), ties=(5, 37), kd_aware=True),
    Config("bsprandomfastkd", _node("bsprandomfastkd"), "attach_bsppaperkd",
           lambda path, tree: _set(bsppaperkd_ref.BspKdScene(path, build=False), tree), film=(36, 15, 24, 12), ties=(12, 59), kd_aware=True),
    Config("bspclusterwithkd", _node("bspclusterwithkd"), "attach_bsppaper",
           lambda path, tree: _set(tree_ref.BspScene(path, build=False), tree), film=(11, 34, 23, 57), ties=(12, 59)),
    Config("kdinst", lambda hprt, m: hprt.KdInst(m), "attach_kdinst",
           lambda path, tree: kdinst_ref.KdInstScene(path).take(tree), film=(12, 30, 22, 50), ties=(59, 122), two_level=True),
    Config("rbspinst13", lambda hprt, m: hprt.RbspInst(m, kd_aware=False, n_directions=13), "attach_rbspinst",
           lambda path, tree: rbspinst_ref.RbspInstScene(path, 13, False).take(tree), film=(22, 12, 30, 6), ties=(59, 122), two_level=True),
    Config("rbspkdinst9", lambda hprt, m: hprt.RbspInst(m, kd_aware=True, n_directions=9), "attach_rbspinst",
           lambda path, tree: rbspinst_ref.RbspInstScene(path, 9, True).take(tree), film=(30, 1, 6, 50), ties=(59, 122), two_level=True,
           kd_aware=True),
]}
FILM_PAIRS = [(c.name, s) for c in CONFIGS.values() for s in c.film]
TIE_PAIRS = [(c.name, s) for c in CONFIGS.values() for s in c.ties]


def bake(hprt, d, text, name):
    """`text` (a random_scene) parsed without warnings and baked under the directory d, which gets the generator's images:
    (model, baked path)"""
    if not (d / "chk.png").exists():
        _write_images(d)
    p = d / (name + ".pbrt")
    p.write_text(text % {"dir": str(d)})
    m = hprt.Model.parse(str(p))
    assert m.warnings() == [], (name, m.warnings())
    path = str(d / (name + ".hprt"))
    m.save(path)
    return m, path


def probe_rays(model, oracle, bounds, seed, n=N_PROBE):
    """two ray families of n rays each, (o, d, tmax): camera rays through random pixels of the film, and tree_walk_checks' random
    rays from inside and around `bounds` (the BVH's six floats), finite and infinite"""
    rng = np.random.default_rng(seed)
    b = np.asarray(bounds, np.float32)
    x0, y0, x1, y1 = model.options.film_bounds()
    oc, dc = oracle.camera_rays(rng.integers(x0, x1, n).astype(np.int32), rng.integers(y0, y1, n).astype(np.int32), rng.integers(0, 2, n).astype(np.int64))
    return (oc, dc, np.full(n, np.inf, np.float32)), twc.random_rays(rng, b[:3], b[3:] - b[:3], n)


def joined(families, n=None):
    """the first n rays (default: all) of each family as one (o, d, tmax)"""
    return tuple(np.concatenate([f[k][:n] for f in families]).astype(np.float32) for k in range(3))


_MATERIAL = re.compile(r'^Material "(\w+)"(.*)$', re.M)
_INSTANCE = re.compile(r"AttributeBegin\n(?:(?!AttributeBegin|AttributeEnd).*\n)*?ObjectInstance")


def traits(text, model):
    """what a generated scene holds, read off its text and its parsed model: the conditions on a config's film seeds are on these"""
    kinds = set()
    for name, rest in _MATERIAL.findall(text):
        if '"color Kd" [0 0 0]' in rest and name == "matte":
            continue                                  # the black body of a sphere or quad emitter: not one of _material's
        if name in ("matte", "plastic") and '"texture Kd"' in rest:
            kinds.add("textured")
        elif name == "matte":
            kinds.add("oren" if '"float sigma"' in rest else "matte")
        else:
            kinds.add(name)
    mirrored = any(re.search(r"^Scale (?:\S+ )*-", blk, re.M) for blk in _INSTANCE.findall(text))
    c = model.counts()
    return {"primitives": c["primitives"], "lights": c["lights"], "sphere": c["spheres"] > 0, "area": "AreaLightSource" in text,
            "infinite": 'LightSource "infinite"' in text, "textures": any('"texture ' in rest for _, rest in _MATERIAL.findall(text)),
            "maxdepth": int(model.options.max_depth),
            "mirrored": mirrored, "materials": kinds}
