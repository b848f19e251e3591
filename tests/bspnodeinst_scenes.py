"""The scenes of the two-level node-based BSP tests (tests/test_bspnodeinst_host.py, tests/test_gpu_bspnodeinst.py): the scene of the
two-level general BSP tests (tests/bsppaperinst_scenes.py) under one of the nine node-based accelerator names, the golden
simple_instanced.hprt, and two degenerate top levels — three instances of one two-triangle object and nothing else, and the same
with a single top-level triangle beside them — on which every primitive the top-level direction choosers see, or all but one, has
a zero normal."""
import os

import bsppaperinst_scenes as bs
import kdinst_scenes as ks
from bsppaperinst_scenes import bake, BLOB, ONE, MIX, LAST, IDENTITY_INSTANCE, N_TOP, N_OBJECTS, N_INSTANCES      # noqa: F401
from bspnode_ref import ACCELERATORS                                                                              # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIMPLE_INSTANCED = os.path.join(GOLDEN, "simple_instanced.hprt")
PAIR = 'ObjectBegin "pair"\n' + ks._mesh([[0, 0, 0], [0.8, 0.1, 0.0], [0.7, 0.9, 0.3], [-0.1, 0.6, 0.2]], [0, 1, 2, 0, 2, 3]) + "ObjectEnd\n"
LONE = ks._mesh([[-1.5, -1.2, 0.1], [1.8, -1.4, 0.3], [0.2, 1.9, -0.2]], [0, 1, 2])


def _named(text, accelerator, accel_params=""):
    assert text.count('Accelerator "bsppaper"') == 1
    return text.replace('Accelerator "bsppaper"', 'Accelerator "%s"%s' % (accelerator, accel_params))


def scene_text(accelerator, accel_params=""):
    """bs.scene_text: 2 floor triangles, a sphere and 8 instances on the top level; objects of 20 triangles, 1 triangle, a sphere
    and 2 triangles, 1 triangle"""
    return _named(bs.scene_text(False), accelerator, accel_params)


def no_instances(accelerator):
    return _named(bs.no_instances(False), accelerator)


def deep_pair(fastkd, object_levels=bs.OBJECT_LEVELS):
    """bs.DeepPair: the hand-made staircases in BSPNode words, or for a fastkd handle in BSPKdNode words (the text's accelerator
    is not read: the tests pass the name)"""
    return bs.DeepPair(fastkd, object_levels)


def only_instances_text(accelerator, lone_triangle=False, accel_params=""):
    """a top level of three instances of one two-triangle object — and, with lone_triangle, one triangle of its own, defined first"""
    return (ks.HEAD.replace('Accelerator "kdtree"%s', 'Accelerator "%s"%s' % (accelerator, accel_params)) + PAIR + (LONE if lone_triangle else "") +
            ks._inst("pair", "Translate -1.1 -0.6 0.2", "Rotate 25 0.1 0.4 1") + ks._inst("pair", "Translate 0.5 -0.2 0.5", "Scale 1.3 0.7 1.6") +
            ks._inst("pair", "Translate -0.2 0.9 0.1", "Scale -1 1 1") + "WorldEnd\n")
