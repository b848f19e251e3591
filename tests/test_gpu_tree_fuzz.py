"""Random scenes through every tree walk on the GPU: the scenes of tests/test_gpu_fuzz.py — every light kind with MIS rays from
area lights and escaped rays into infinite lights, every material with glass and mirror chains, image textures, partial spheres,
(two-level) spheres and textured meshes inside mirrored instances, odd resolutions and crop windows, maxdepth 0-12 — rendered with
a tree attached instead of the BVH, for the (config, seed) pairs of tests/tree_fuzz.py, whose input conditions
tests/test_tree_fuzz_host.py holds on the CPU.

On a FILM pair the walk is held to its test-side restatement over the same tree — closest hits, any-hit flags, the four counters
and for kd-aware trees the kd share, on camera, random and degenerate rays — and the render to the CPU oracle's: the film in
every bit and the ray counts of a counting render.  The restatement finds the oracle's hit on these scenes (no ties), so a film
that differs is the walk's epilogue or the way the render drives it: the queues, the any-hit walk's result on the way to
k_repair, the closest-hit walk on the MIS stream.  The same film comes from the counting render, a poisoned workspace, odd batch
cuts, the old path of the light samples (every pending term through k_resolve), two tile shards merged and a render with
per-pixel statistics, whose sums are the render's counters.  Every third seed fills its light-distribution voxels on demand
(the retry pass).  The first film seed of each config was chosen, by the counts of the unattached BVH scene, to have speculated
vertices that were repaired, ones that were not, and vertices with an MIS ray.

On a TIE pair coincident surfaces are settled by the traversal order: the walk returns the restatement's choice on every ray, at
the BVH's t."""
import os

import numpy as np
import pytest

import tree_fuzz as tf
import tree_walk_checks as twc
from test_gpu_kdinst import check_parity as check_kdinst_parity
from test_gpu_rbspinst import check_parity as check_rbspinst_parity
from test_gpu_speculated_light import _counting, _counts, _old_path, _same

pytestmark = pytest.mark.gpu


class _Case:
    def __init__(self, hprt, orc, d, name, seed, tie):
        c = self.config = tf.CONFIGS[name]
        self.name, self.seed, self.tie = name, seed, tie
        self.first = not tie and seed == c.film[0]
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
            self.bvh_t = self.scene.intersect_instanced(*tf.joined(self.rays[:2]))[0]      # (before the tree takes the scene over)
        self.tree = c.make(hprt, self.model)
        getattr(self.scene, c.attach)(self.tree)
        self.ref = c.restate(self.path, self.tree)


def _ids(pairs):
    return ["%s-%d" % p for p in pairs]


@pytest.fixture(scope="module", params=tf.FILM_PAIRS, ids=_ids(tf.FILM_PAIRS))
def film_case(request, hprt, orc, tmp_path_factory):
    return _Case(hprt, orc, tmp_path_factory.mktemp("tree_fuzz"), *request.param, False)


@pytest.fixture(scope="module", params=tf.TIE_PAIRS, ids=_ids(tf.TIE_PAIRS))
def tie_case(request, hprt, orc, tmp_path_factory):
    return _Case(hprt, orc, tmp_path_factory.mktemp("tree_fuzz"), *request.param, True)


def _check_walk(case):
    """hprt_intersect_instanced / hprt_intersect / hprt_occluded with counting on against the restated walk over the same tree;
    returns the restatement's t on the joined rays"""
    c, sc, ref = case.config, case.scene, case.ref
    o, d, tm = tf.joined(case.rays)
    if c.two_level:
        check = check_rbspinst_parity if c.attach == "attach_rbspinst" else check_kdinst_parity
        t0, p0, i0 = check(sc, ref, o, d, tm)
        assert (i0 >= 0).any() and ((p0 >= 0) & (i0 < 0)).any() and (p0 < 0).any()      # inside instances, on the top level, misses
        return t0
    twc.check_closest(sc, ref, case.rays)
    twc.check_any(sc, ref, case.rays)
    t0, p0, b0, _ = ref.intersect(o, d, tm)
    t1, p1, i1, b1 = sc.intersect_instanced(o, d, tm)          # the entry point with the instance: the same walk, and no instance
    assert np.array_equal(p0, p1) and np.array_equal(twc._bits(t0), twc._bits(t1)) and np.array_equal(twc._bits(b0), twc._bits(b1))
    assert (i1 == -1).all() and (p0 >= 0).any() and (p0 < 0).any()
    return t0


def test_walk_equals_the_restatement(film_case):
    _check_walk(film_case)


def test_film_equals_the_oracle(hprt, film_case):
    case, c, sc, m = film_case, film_case.config, film_case.scene, film_case.model
    what = "%s, seed %d" % (case.name, case.seed)
    _, film0, c0, _, _ = case.oracle.render(threads=8)
    film0.setflags(write=False)
    assert film0[..., :3].max() > 0 and c0["shadow_rays"] > 0
    # the plain render; on a config's first seed with the speculation counted: both outcomes of k_repair after the tree's any-hit
    # trace, and vertices whose MIS ray the closest-hit walk traces
    if case.first:
        _counting(hprt, sc, True)
    plain, st = sc.render()
    if case.first:
        speculated, repaired, full = _counts(hprt, sc)
        _counting(hprt, sc, False)
        print("%s: speculated %d, repaired %d, full %d" % (what, speculated, repaired, full))
    _same(plain, film0, what)
    if case.first:
        assert repaired > 0 and speculated > repaired and full > 0, (speculated, repaired, full)
    # the counting render: the reference's full ray set (the node counters are the tree's here, the oracle's the BVH's)
    counted, stc = sc.render(count_work=True)
    _same(counted, film0, what + " (counting)")
    for k in ("camera_rays", "rays", "shadow_rays"):
        assert stc[k] == c0[k], (what, k, stc[k], c0[k])
    assert st["rays"] <= stc["rays"]
    sc.debug_poison(0xFF)
    try:
        poisoned, _ = sc.render()
    finally:
        sc.debug_poison(None)
    _same(poisoned, film0, what + " (poisoned)")
    opt = m.options.copy()
    cut, _ = sc.render(opt, spp_chunk=max(1, opt.spp // 3))
    _same(cut, film0, what + " (spp_chunk)")
    with _old_path(hprt):
        old, st_old = sc.render()
    _same(old, film0, what + " (old path)")
    assert (st_old["rays"], st_old["shadow_rays"]) == (st["rays"], st["shadow_rays"])
    merged = np.zeros_like(plain)
    records = []
    for r in range(2):
        part, _ = sc.render(opt, tile_begin=r, tile_stride=2, export_foreign=True)
        merged += part
        records.append(sc.film_records())
    hprt.film_records_merge(merged, np.concatenate(records[::-1]))
    _same(merged, film0, what + " (two shards)")
    # per-pixel statistics (a counting render too): the same film, and the pixels' sums are the render's counters
    # (tree_walk_checks.check_counting_render)
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
        assert kdc == (0, 0)


def test_ties_go_the_restatements_way(tie_case):
    t0 = _check_walk(tie_case)
    n = 2 * tf.N_PROBE_GPU          # the probe rays; the BVH walk turns a degenerate ray's NaN away where a tree walk "hits" at NaN
    assert np.array_equal(twc._bits(t0[:n]), twc._bits(tie_case.bvh_t))
