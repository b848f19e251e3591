"""The scenes of the two-level general BSP tests (tests/test_bsppaperinst_host.py, tests/test_gpu_bsppaperinst.py): the scene of the
two-level RBSP tests (tests/rbspinst_scenes.py, itself tests/kdinst_scenes.py's) with the Accelerator line replaced by "bsppaper" /
"bsppaperkd" and two additions — an instance of the all-triangle object under the IDENTITY transform, so that rays built in its
object space from the copied object tree are world rays too, and a one-primitive object defined LAST, whose stand-in leaf is then
the last node of the attached node array and its axis entry the last of the axis array — the tie and no-instance texts, and the
deep pair of staircases in their general BSP encodings."""
import numpy as np

import kdinst_scenes as ks
from kdinst_scenes import bake, TOP_LEVELS, OBJECT_LEVELS      # noqa: F401  (the tests take them from here)
from rbspinst_scenes import blob_triangles                     # noqa: F401

BLOB, ONE, MIX, LAST = 0, 1, 2, 3           # object definitions in order
IDENTITY_INSTANCE = 6                       # the blob under no transform
N_TOP, N_OBJECTS, N_INSTANCES = 2 + 1 + 8, 4, 8
LAST_OBJECT = 'ObjectBegin "last"\n' + ks._mesh([[0, 0, 0], [0.5, 0.1, 0.0], [0.1, 0.5, 0.2]], [0, 1, 2]) + "ObjectEnd\n"      # object 3: one triangle, no tree


def accel(kd_aware):
    return 'Accelerator "%s"' % ("bsppaperkd" if kd_aware else "bsppaper")


def _with(text, kd_aware):
    assert text.count('Accelerator "kdtree"') == 1
    return text.replace('Accelerator "kdtree"', accel(kd_aware))


def scene_text(kd_aware, accel_params=""):
    """ks.scene_text — two floor triangles, a top-level sphere, the blob under three transforms, the one-triangle object twice, the
    sphere-and-triangles object once — with the last object defined after the others and, as the last two instances, the blob
    under the identity and the last object; accel_params follow the accelerator's name"""
    text = ks.scene_text(accel_params)
    assert text.count(ks.MIX) == 1 and text.endswith("WorldEnd\n")
    text = text.replace(ks.MIX, ks.MIX + LAST_OBJECT)
    text = text[:-len("WorldEnd\n")] + ks._inst("blob") + ks._inst("last", "Translate 1.4 1.6 0.3", "Rotate 20 0 0 1") + "WorldEnd\n"
    return _with(text, kd_aware)


def tie_text(kd_aware):
    return _with(ks.tie_text(), kd_aware)


def no_instances(kd_aware):
    return _with(ks.NO_INSTANCES, kd_aware)


class DeepPair(ks.DeepPair):
    """ks.DeepPair with the staircases' general BSP encodings, 5 words per node: Staircase.bsppaper() (every node takes the
    dot-product step against its own axis) or, kd-aware, Staircase.bsppaperkd() (kd and plane nodes alternate level by level).
    5 + 58 + 1 = 64 levels as there."""

    def __init__(self, kd_aware, object_levels=OBJECT_LEVELS):
        ks.DeepPair.__init__(self, object_levels)
        self.kd_aware = kd_aware

    def text(self):
        return _with(ks.DeepPair.text(self), self.kd_aware)

    def trees(self):
        """{-1: (nodes, idx) of the top level, 0: of the object}"""
        out = {}
        for obj, stairs in ((-1, self.top), (0, self.obj)):
            nodes, idx = stairs.bsppaperkd() if self.kd_aware else stairs.bsppaper()
            if obj < 0:       # the top level's only many-primitive leaf is its last: the instance first, before a triangle there can shorten the ray
                assert idx.tolist() == [2 * TOP_LEVELS - 1, 2 * TOP_LEVELS, 2 * TOP_LEVELS + 1]
                idx = np.roll(idx, 1)
            out[obj] = (nodes, idx)
        return out

    def install(self, bspinst, ref):
        """the two hand-made trees in the library's handle and in the restatement, each with the union of its primitives' bounds"""
        for obj, (nodes, idx) in self.trees().items():
            bspinst.set_tree(obj, nodes, idx, ref.tree_bounds(obj))
            ref.set_tree(obj, nodes, idx)
