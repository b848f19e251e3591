"""The scenes of the two-level kd-tree tests (tests/test_kdinst_host.py, tests/test_gpu_kdinst.py): a small instanced scene as .pbrt
text (parsed and baked, so that model, oracle and restatement load one file), its tie variant, and the deep pair of staircases."""
import os

import numpy as np

import deep_todo

HEAD = """LookAt 3.2 -4.5 3.0  0 0.1 0.3  0 0 1
Camera "perspective" "float fov" [42]
Film "image" "integer xresolution" [64] "integer yresolution" [48]
Sampler "halton" "integer pixelsamples" [2]
Integrator "path" "integer maxdepth" [3]
Accelerator "kdtree"%s
WorldBegin
LightSource "point" "point from" [0.5 -1 6] "color I" [40 40 40]
"""


def _blob():
    """20 triangles: a 5 x 2 grid of quads over [0, 1] x [0, 0.6] with a bumpy z, no two triangles coplanar neighbours' duplicates"""
    rng = np.random.default_rng(7)
    xs, ys = np.linspace(0, 1, 6), np.linspace(0, 0.6, 3)
    P = np.array([[x, y, 0.25 * rng.uniform()] for y in ys for x in xs], np.float32)
    idx = []
    for j in range(2):
        for i in range(5):
            a, b, c, d = j * 6 + i, j * 6 + i + 1, (j + 1) * 6 + i + 1, (j + 1) * 6 + i
            idx += [a, b, c, a, c, d]
    return P, idx


def _mesh(P, idx):
    return 'Shape "trianglemesh" "integer indices" [%s] "point P" [%s]\n' % (" ".join(map(str, idx)), " ".join(repr(float(v)) for v in np.asarray(P).ravel()))


BLOB = 'ObjectBegin "blob"\n' + _mesh(*_blob()) + "ObjectEnd\n"                     # object 0: 20 triangles
ONE = 'ObjectBegin "one"\n' + _mesh([[0, 0, 0], [0.7, 0, 0.1], [0.1, 0.6, 0.3]], [0, 1, 2]) + "ObjectEnd\n"      # object 1: one triangle, no tree
MIX = ('ObjectBegin "mix"\nAttributeBegin\nTranslate 0.1 0.1 0.3\nShape "sphere" "float radius" [0.25]\nAttributeEnd\n' +
       _mesh([[-0.4, -0.3, 0], [0.5, -0.3, 0.05], [0.5, 0.5, 0], [-0.4, 0.5, 0.1]], [0, 1, 2, 0, 2, 3]) + "ObjectEnd\n")     # object 2: a sphere and two triangles
FLOOR = _mesh([[-3, -3, -0.1], [3, -3, -0.1], [3, 3, -0.1], [-3, 3, -0.1]], [0, 1, 2, 2, 3, 0])


def _inst(name, *xf):
    return "AttributeBegin\n" + "".join(x + "\n" for x in xf) + 'ObjectInstance "%s"\nAttributeEnd\n' % name


def scene_text(accel_params=""):
    """Two floor triangles, a top-level sphere, the blob instanced under a rotation, a non-uniform scale and a mirroring scale, the
    one-triangle object twice, the sphere-and-triangles object once.  No two surfaces coincide."""
    return (HEAD % accel_params + BLOB + ONE + MIX + FLOOR +
            'AttributeBegin\nTranslate 0.2 0.1 0.6\nShape "sphere" "float radius" [0.35]\nAttributeEnd\n' +
            _inst("blob", "Translate -1.6 -0.9 0.2", "Rotate 35 0.2 0.3 1") +
            _inst("blob", "Translate 0.4 -1.3 0.3", "Scale 1.5 0.6 2.0") +
            _inst("blob", "Translate 2.0 0.7 0.4", "Scale -1 1 1.2") +
            _inst("one", "Translate -0.6 1.0 0.5") +
            _inst("one", "Translate 0.5 1.3 0.8", "Rotate 50 1 0 0") +
            _inst("mix", "Translate -1.6 0.7 0.5") + "WorldEnd\n")


def tie_text():
    """Two instances of the blob (and two of the one-triangle object) under the same transform: every triangle of the one coincides
    with a triangle of the other, so every hit on them is a tie between two instances."""
    return (HEAD % "" + BLOB + ONE + FLOOR +
            _inst("blob", "Translate -0.5 -0.4 0.3", "Scale 1.5 1.5 1.5") + _inst("blob", "Translate -0.5 -0.4 0.3", "Scale 1.5 1.5 1.5") +
            _inst("one", "Translate 0.2 0.8 0.4") + _inst("one", "Translate 0.2 0.8 0.4") + "WorldEnd\n")


NO_INSTANCES = HEAD % "" + FLOOR + "WorldEnd\n"


def bake(hprt, directory, text, name):
    """(model, path of the baked scene) of a .pbrt text"""
    stem = os.path.join(str(directory), name)
    with open(stem + ".pbrt", "w") as f:
        f.write(text)
    m = hprt.Model.parse(stem + ".pbrt")
    m.save(stem + ".hprt")
    return m, stem + ".hprt"


# ---- the deep pair: a short top-level staircase whose last leaf holds an instance of a long one ----
TOP_LEVELS, OBJECT_LEVELS = 5, 58          # 5 + 58 + 1 = 64: the capacity hprt_scene_attach_kdinst accepts


class DeepPair:
    """deep_todo.Staircase(TOP_LEVELS) as the top-level triangles, with the instance as the primitive after them — tested in the
    last leaf, where a ray of the deep family holds TOP_LEVELS entries — and Staircase(object_levels) as the object, translated so
    that its last slab lies where the top level's does: the ray enters the instance beyond the object's last plane too and pushes
    object_levels more entries above the saved position.  (The 0.05 keeps the two staircases' triangle planes apart.)"""

    def __init__(self, object_levels=OBJECT_LEVELS):
        self.top = deep_todo.Staircase(TOP_LEVELS, seed=3, sphere=True)      # (sphere=True: its layout puts primitive 2 L + 1 in the last leaf — here the instance)
        self.obj = deep_todo.Staircase(object_levels, seed=4)
        self.shift = TOP_LEVELS - object_levels + 0.05

    def text(self):
        L = TOP_LEVELS
        return ("LookAt %r 0.05 0.1  0 0 0  0 0 1\n" % float(L + 2.0) +
                'Camera "perspective" "float fov" [12]\nFilm "image" "integer xresolution" [64] "integer yresolution" [64]\n'
                'Sampler "halton" "integer pixelsamples" [2]\nIntegrator "path" "integer maxdepth" [3]\nAccelerator "kdtree"\nWorldBegin\n'
                'LightSource "point" "point from" [%r 0 0] "color I" [400 400 400]\n' % float(L + 1.0) +
                'ObjectBegin "stairs"\n' + _mesh(self.obj.tris.reshape(-1, 3), range(3 * self.obj.tris.shape[0])) + "ObjectEnd\n" +
                _mesh(self.top.tris.reshape(-1, 3), range(3 * self.top.tris.shape[0])) +
                _inst("stairs", "Translate %r 0 0" % self.shift) + "WorldEnd\n")

    def install(self, kdinst, ref):
        """the two hand-made trees in the library's handle and in the restatement, each with the union of its primitives' bounds"""
        for obj, stairs in ((-1, self.top), (0, self.obj)):
            nodes, idx = stairs.kdtree()
            if obj < 0:       # the top level's only many-primitive leaf is its last: the instance first, before a triangle there can shorten the ray
                assert idx.tolist() == [2 * TOP_LEVELS - 1, 2 * TOP_LEVELS, 2 * TOP_LEVELS + 1]
                idx = np.roll(idx, 1)
            kdinst.set_tree(obj, nodes, idx, ref.tree_bounds(obj))
            ref.set_tree(obj, nodes, idx)

    STOPS = (1, 2, 3, 4, 5, 10, 26, 57)        # object levels a finite tMax stops the object's descent at

    def deep_rays(self, n):
        """The OBJECT staircase's deep family (deep_todo.Staircase.deep_rays: from beyond the last plane, d.x < 0, aimed along the whole
        staircase so that it stays inside the object's bounds) moved to world space: it starts beyond the top level's last plane too.
        Even rays have tMax = inf and hold every entry of both levels at the object's first leaf: TOP_LEVELS + 1 + object levels.
        Odd rays end half a slab beyond the object's plane (levels - j), j from STOPS in turn: the object pushes j entries, the top
        level those of its planes the ray still reaches, so the totals fall on both sides of the walk's LDS count."""
        o, d, _, _ = self.obj.deep_rays(n)
        o = (o + np.array([self.shift, 0, 0])).astype(np.float32)
        i = np.arange(n)
        j = np.array(self.STOPS)[(i // 2) % len(self.STOPS)]
        stop_x = (self.obj.L - j) - 0.5 + self.shift
        tm = np.where(i % 2 == 0, np.inf, (stop_x - o[:, 0].astype(np.float64)) / d[:, 0].astype(np.float64)).astype(np.float32)
        return o, d, tm
