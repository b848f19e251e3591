"""Random instanced scenes through the two-level general BSP walks on the GPU: what tests/test_gpu_tree_fuzz.py does for the eleven
other walks, for the (config, seed) pairs of tests/bsppaperinst_fuzz.py, whose input conditions tests/test_bsppaperinst_fuzz_host.py
holds on the CPU.

On a FILM pair the walk is held to its test-side restatement over the same trees — closest hits with their instance, any-hit flags,
the four counters and for kd-aware trees the kd share, on 4,096 camera, 4,096 random and 4,096 degenerate rays — and the render to
the CPU oracle's: the film in every bit, plain, counting (with the oracle's ray counts) and with per-pixel statistics, whose sums
are the render's counters.  The restatement finds the oracle's hit on these scenes (no ties), so a film that differs is the walk's
epilogue or the way the render drives it.  On a TIE pair coincident surfaces are settled by the traversal order: the walk returns
the restatement's choice on every ray, at the BVH's t."""
import os

import numpy as np
import pytest

import bsppaperinst_fuzz as bf
import tree_fuzz as tf
import tree_walk_checks as twc
from test_gpu_rbspinst import check_parity
from test_gpu_speculated_light import _same

pytestmark = pytest.mark.gpu


class _Case:
    """tests/test_gpu_tree_fuzz.py's, with the config looked up here"""

    def __init__(self, hprt, orc, d, name, seed, tie):
        c = self.config = bf.CONFIGS[name]
        self.name, self.seed, self.tie = name, seed, tie
        self.model, self.path = tf.bake(hprt, d, c.text(seed, tie), "%s_%d_%s" % (name, seed, "tie" if tie else "film"))
        self.oracle = orc.OracleScene(self.path)
        bvh = hprt.Bvh(self.model)
        self.bounds = np.array(bvh.info()["bounds"], np.float32)
        # every third seed builds its spatial light distribution on demand (voxel rows as the vertices ask for them + the retry pass)
        if seed % 3 == 0:
            os.environ["HPRT_VOXEL_DENSE_MAX_MB"] = "0"
        try:
            self.scene = hprt.Scene(self.model, bvh)
        finally:
            os.environ.pop("HPRT_VOXEL_DENSE_MAX_MB", None)
        probes = tf.probe_rays(self.model, self.oracle, self.bounds, seed)
        blo, ext = self.bounds[:3], self.bounds[3:] - self.bounds[:3]
        self.rays = [tuple(a[:tf.N_PROBE_GPU] for a in f) for f in probes] + [twc.degenerate_rays(np.random.default_rng(seed + 1000), blo, ext, tf.N_PROBE_GPU)]
        if tie:
            self.bvh_t = self.scene.intersect_instanced(*tf.joined(self.rays[:2]))[0]      # (before the trees take the scene over)
        self.tree = c.make(hprt, self.model)
        getattr(self.scene, c.attach)(self.tree)
        self.ref = c.restate(self.path, self.tree)


def _ids(pairs):
    return ["%s-%d" % p for p in pairs]


@pytest.fixture(scope="module", params=bf.FILM_PAIRS, ids=_ids(bf.FILM_PAIRS))
def film_case(request, hprt, orc, tmp_path_factory):
    return _Case(hprt, orc, tmp_path_factory.mktemp("bsppaperinst_fuzz"), *request.param, False)


@pytest.fixture(scope="module", params=bf.TIE_PAIRS, ids=_ids(bf.TIE_PAIRS))
def tie_case(request, hprt, orc, tmp_path_factory):
    return _Case(hprt, orc, tmp_path_factory.mktemp("bsppaperinst_fuzz"), *request.param, True)


def _check_walk(case):
    """hprt_intersect_instanced / hprt_intersect / hprt_occluded with counting on against the restated walk over the same trees;
    returns the restatement's t on the joined rays"""
    t0, p0, i0 = check_parity(case.scene, case.ref, *tf.joined(case.rays))
    assert (i0 >= 0).any() and ((p0 >= 0) & (i0 < 0)).any() and (p0 < 0).any()      # inside instances, on the top level, misses
    return t0


def test_walk_equals_the_restatement(film_case):
    _check_walk(film_case)


def test_film_equals_the_oracle(film_case):
    case, c, sc = film_case, film_case.config, film_case.scene
    what = "%s, seed %d" % (case.name, case.seed)
    _, film0, c0, _, _ = case.oracle.render(threads=8)
    film0.setflags(write=False)
    assert film0[..., :3].max() > 0 and c0["shadow_rays"] > 0
    plain, st = sc.render()
    _same(plain, film0, what)
    # the counting render: the reference's full ray set (the node counters are the trees' here, the oracle's the BVH's)
    counted, stc = sc.render(count_work=True)
    _same(counted, film0, what + " (counting)")
    for k in ("camera_rays", "rays", "shadow_rays"):
        assert stc[k] == c0[k], (what, k, stc[k], c0[k])
    assert st["rays"] <= stc["rays"]
    # per-pixel statistics (a counting render too): the same film, and the pixels' sums are the render's counters
    stats_film, stp = sc.render(pixel_stats=True)
    _same(stats_film, film0, what + " (pixel statistics)")
    s = sc.pixel_stats().reshape(-1, 7).sum(0)
    assert s[5] > 0 and s[6] > 0 and s[3] > 0
    assert s[5] == stp["nodes_entered"] and s[6] == stp["nodes_entered_p"]
    assert s[3] + s[5] == stp["nodes_fetched"] and s[4] + s[6] == stp["nodes_fetched_p"]
    assert s[1] == stp["tri_tests"] + stp["sphere_tests"] and s[2] == stp["tri_tests_p"] + stp["sphere_tests_p"]
    assert (stp["camera_rays"], stp["rays"], stp["shadow_rays"]) == (c0["camera_rays"], c0["rays"], c0["shadow_rays"])
    kdc = sc.kd_counters()
    if c.kd_aware:
        kd2 = sc.pixel_kd_stats()
        assert (int(kd2[0].sum()), int(kd2[1].sum())) == kdc and kdc[0] > 0 and kdc[1] > 0
    else:
        assert kdc == (0, 0) and not sc.pixel_kd_stats().any()


def test_ties_go_the_restatements_way(tie_case):
    t0 = _check_walk(tie_case)
    n = 2 * tf.N_PROBE_GPU          # the probe rays; the BVH walk turns a degenerate ray's NaN away where a tree walk "hits" at NaN
    assert np.array_equal(twc._bits(t0[:n]), twc._bits(tie_case.bvh_t))
