"""The scenes of the two-level RBSP tests (tests/test_rbspinst_host.py, tests/test_gpu_rbspinst.py): those of the two-level kd-tree
tests (tests/kdinst_scenes.py) with Accelerator "kdtree" replaced by "rbsp" / "rbspkd" and "integer nbDirections", and the deep
pair of staircases in their RBSP encodings."""
import numpy as np

import deep_todo
import kdinst_scenes as ks
from kdinst_scenes import bake, TOP_LEVELS, OBJECT_LEVELS      # noqa: F401  (the tests take them from here)


def accel(kd_aware, M):
    return 'Accelerator "%s" "integer nbDirections" [%d]' % ("rbspkd" if kd_aware else "rbsp", M)


def _with(text, kd_aware, M):
    assert text.count('Accelerator "kdtree"') == 1
    return text.replace('Accelerator "kdtree"', accel(kd_aware, M))


def scene_text(kd_aware, M, accel_params=""):
    """ks.scene_text: two floor triangles, a top-level sphere, the blob under three transforms, the one-triangle object twice, the
    sphere-and-triangles object once; accel_params follow "nbDirections" on the Accelerator line"""
    return _with(ks.scene_text(accel_params), kd_aware, M)


def tie_text(kd_aware, M):
    return _with(ks.tie_text(), kd_aware, M)


def no_instances(kd_aware, M):
    return _with(ks.NO_INSTANCES, kd_aware, M)


def blob_triangles():
    """[20, 9]: the object-space triangles of the all-triangle object (object 0), in creation order"""
    P, idx = ks._blob()
    return P[np.array(idx)].reshape(-1, 9).astype(np.float32)


class DeepPair(ks.DeepPair):
    """ks.DeepPair with the staircases' RBSP encodings: Staircase.rbsp() (M = 7: every node takes the dot-product step) or, kd-aware,
    Staircase.rbspkd() (M = 9: the chain are kd nodes, the siblings of odd levels oblique).  5 + 58 + 1 = 64 levels as there."""

    def __init__(self, kd_aware, object_levels=OBJECT_LEVELS):
        ks.DeepPair.__init__(self, object_levels)
        self.kd_aware = kd_aware
        self.M = deep_todo.RBSPKD_M if kd_aware else deep_todo.RBSP_M

    def text(self):
        return _with(ks.DeepPair.text(self), self.kd_aware, self.M)

    def trees(self):
        """{-1: (nodes, idx) of the top level, 0: of the object}"""
        out = {}
        for obj, stairs in ((-1, self.top), (0, self.obj)):
            nodes, idx = stairs.rbspkd() if self.kd_aware else stairs.rbsp()
            if obj < 0:       # the top level's only many-primitive leaf is its last: the instance first, before a triangle there can shorten the ray
                assert idx.tolist() == [2 * TOP_LEVELS - 1, 2 * TOP_LEVELS, 2 * TOP_LEVELS + 1]
                idx = np.roll(idx, 1)
            out[obj] = (nodes, idx)
        return out

    def install(self, rbspinst, ref):
        """the two hand-made trees in the library's handle and in the restatement, each with the union of its primitives' bounds"""
        for obj, (nodes, idx) in self.trees().items():
            rbspinst.set_tree(obj, nodes, idx, ref.tree_bounds(obj))
            ref.set_tree(obj, nodes, idx)
