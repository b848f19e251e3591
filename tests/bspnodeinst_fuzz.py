"""The tie-free seeds of the two-level node-based walks: two more tree_fuzz.Config over the instanced random
scenes (random_scene(seed, objects=2)), for "bsprandom" and "bsprandomfastkd" at K = 5 with the tree seed 7 — the two forms whose
trees lose no hit.  (The arbitrary and cluster choosers hand out a primitive's own normal as a split direction, and a triangle
lying in its own split plane is lost: §8f's finding.  Those forms are compared with the restatement only.)

tests/test_bspnodeinst_host.py asserts on the CPU that every committed (config, seed) pair is an input: on 20,000 camera rays and
20,000 random rays the restated two-level walk over the library's trees finds the oracle's closest hit — primitive, instance, the
bits of t and of the barycentrics.  tests/test_gpu_bspnodeinst.py holds the films of these pairs to the BVH's.  The seeds are the
two-level film seeds of tests/bsppaperinst_fuzz.py; all of them met the condition, none was replaced.  None of it measures a device
walk."""
import bsppaperinst_ref
import tree_fuzz as tf

K, TREE_SEED = tf.NODE_K, tf.NODE_SEED


def _make(accelerator):
    return lambda hprt, m: hprt.BspNodeInst(m, accelerator, n_directions=K, seed=TREE_SEED)


CONFIGS = {c.name: c for c in [
    tf.Config("bsprandominst", _make("bsprandom"), "attach_bsppaperinst",
              lambda path, tree: bsppaperinst_ref.BspPaperInstScene(path, False).take(tree), film=(12, 22, 30, 6), ties=(), two_level=True),
    tf.Config("bsprandomfastkdinst", _make("bsprandomfastkd"), "attach_bsppaperinst",
              lambda path, tree: bsppaperinst_ref.BspPaperInstScene(path, True).take(tree), film=(30, 1, 6, 50), ties=(), two_level=True,
              kd_aware=True),
]}
FILM_PAIRS = [(c.name, s) for c in CONFIGS.values() for s in c.film]
