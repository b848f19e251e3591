"""The tree fuzz (tests/tree_fuzz.py) for the two-level general BSP walks: two more tree_fuzz.Config over the
instanced random scenes (objects=2), plain and kd-aware, with seed lists of their own.  tests/test_bsppaperinst_fuzz_host.py holds
the input conditions on the CPU, tests/test_gpu_bsppaperinst_fuzz.py the walk and the films on the GPU.

The seeds were picked on the CPU by the conditions the host test asserts, starting from the two-level seeds already in use (film
12, 22, 30, 6, 1, 50; ties 59, 122) so that a scene is parsed and rendered by the oracle once for all two-level walks; none of
them is a measurement of the device walk.  The restatement walks the LIBRARY's trees (take)."""
import bsppaperinst_ref
import tree_fuzz as tf

CONFIGS = {c.name: c for c in [
    tf.Config("bsppaperinst", lambda hprt, m: hprt.BspPaperInst(m, kd_aware=False, isect_cost=80), "attach_bsppaperinst",
              lambda path, tree: bsppaperinst_ref.BspPaperInstScene(path, False).take(tree), film=(12, 22, 30, 6), ties=(59, 122), two_level=True),
    tf.Config("bsppaperkdinst", lambda hprt, m: hprt.BspPaperInst(m, kd_aware=True, isect_cost=80), "attach_bsppaperinst",
              lambda path, tree: bsppaperinst_ref.BspPaperInstScene(path, True).take(tree), film=(30, 1, 6, 50), ties=(59, 122), two_level=True,
              kd_aware=True),
]}
FILM_PAIRS = [(c.name, s) for c in CONFIGS.values() for s in c.film]
TIE_PAIRS = [(c.name, s) for c in CONFIGS.values() for s in c.ties]
