"""Two-level node-based BSP trees on the GPU (hprt.BspNodeInst under hprt_scene_attach_bsppaperinst and k_bsppaperinstwalk<..., KD>,
both unchanged): closest and any hit held bit for bit to the test-side two-level walk (tests/bsppaperinst_reference.cpp) over the
library's trees — t, primitive, instance, barycentrics, the four counters and the kd share — for all nine accelerator names at
K = 5, on the scene of tests/bspnodeinst_scenes.py, on tests/golden/simple_instanced.hprt and on rays that start on the split planes
of an object's tree; the films of the tie-free seeds (tests/bspnodeinst_fuzz.py) against the BVH's film; four two-level attaches in
turn on one scene; and the device-assisted build (hprt_bspnodeinst_build_device) against the host's bytes.  The trees themselves are
held to the restated builds on the CPU (tests/test_bspnodeinst_host.py).  Nothing here has a tolerance."""
import numpy as np
import pytest

import bspnodeinst_fuzz as nf
import bspnodeinst_ref as nr
import bspnodeinst_scenes as ns
import bsppaperinst_ref
import kdinst_ref
import kdinst_scenes as ks
import rbspinst_ref
import tree_fuzz as tf
from test_gpu_bsppaperinst import _on_plane_rays
from test_gpu_kdinst import check_parity as check_kd_parity
from test_gpu_rbspinst import _rays, check_parity

pytestmark = pytest.mark.gpu
ACCS = ns.ACCELERATORS
K, SEED = 5, 7


class _Case:
    """the trees of one accelerator name over a model, their restated walk, and (attach=True) a device scene that walks them"""

    def __init__(self, hprt, orc, m, path, acc, attach=True):
        self.m, self.path, self.acc, self.kd = m, path, acc, nr.fastkd(acc)
        self.trees = hprt.BspNodeInst(m, acc, n_directions=K, seed=SEED)
        self.ref = bsppaperinst_ref.BspPaperInstScene(path, self.kd).take(self.trees)
        self.oracle = orc.OracleScene(path)
        if attach:
            self.sc = hprt.Scene(m, hprt.Bvh(m), device=0)
            self.sc.attach_bsppaperinst(self.trees)

    def rays(self, n, seed):
        return _rays(self.m, self.ref, self.oracle, n, seed)


@pytest.fixture(scope="module")
def own_scene(hprt, tmp_path_factory):
    return ns.bake(hprt, tmp_path_factory.mktemp("bspnodeinst"), ns.scene_text("bspcluster"), "scene")


@pytest.fixture(scope="module", params=ACCS)
def own(request, hprt, orc, own_scene):
    return _Case(hprt, orc, *own_scene, request.param)


def test_hits_equal_the_reference_walk_on_the_test_scene(own):
    o, d, tm = own.rays(20000, 1)
    assert np.isinf(tm).any() and np.isfinite(tm).any()
    t, p, inst = check_parity(own.sc, own.ref, o, d, tm)
    # (the arbitrary and cluster trees lose hits by construction; what is held is the restatement over the same trees)
    assert (inst >= 0).any() and (p < 0).any() and ((p >= 0) & (inst < 0)).any()
    if own.acc.startswith("bsprandom"):
        assert set(np.unique(inst).tolist()) == {-1} | set(range(ns.N_INSTANCES))


def test_rays_that_start_on_a_split_plane_of_the_identity_instances_object_tree(own):
    """2,048 rays in the object space of the all-triangle object (world space for its identity instance) with float
    Dot(axis, o) == split of one of its plane nodes and Dot(axis, d) == 0 exactly; for a fastkd tree as many again on a kd node's
    split with d[axis] = +-0 (tests/test_gpu_bsppaperinst.py builds them)"""
    families = _on_plane_rays(own, 2048, np.random.default_rng(11))
    assert len(families) == (2 if own.kd else 1)
    reached = False
    for o, d, tm in families:
        assert o.shape[0] == 2048
        t, p, inst = check_parity(own.sc, own.ref, o, d, tm)
        reached |= bool((inst == ns.IDENTITY_INSTANCE).any())
    assert reached


@pytest.mark.parametrize("acc", ACCS)
def test_hits_equal_the_reference_walk_on_simple_instanced(hprt, orc, acc):
    """the golden scene whose top level holds only the instance"""
    case = _Case(hprt, orc, hprt.Model.load(ns.SIMPLE_INSTANCED), ns.SIMPLE_INSTANCED, acc)
    _, p, inst = check_parity(case.sc, case.ref, *case.rays(20000, 3))
    assert (inst >= 0).any() and (p < 0).any()


@pytest.mark.parametrize("name,seed", nf.FILM_PAIRS, ids=["%s-%d" % p for p in nf.FILM_PAIRS])
def test_tie_free_film_equals_the_bvh_film(hprt, tmp_path, name, seed):
    """the trees of these pairs lose no hit (tests/test_bspnodeinst_host.py): the render through them is the BVH's render in every
    bit — plain, counting and with per-pixel statistics, whose sums are the render's counters; fastkd: the kd share per pixel"""
    c = nf.CONFIGS[name]
    m, _ = tf.bake(hprt, tmp_path, c.text(seed), "%s_%d" % (name, seed))
    sc = hprt.Scene(m, hprt.Bvh(m), device=0)
    film0, _ = sc.render()
    counted0, st0 = sc.render(count_work=True)
    assert np.isfinite(film0).all() and film0[..., :3].max() > 0 and st0["shadow_rays"] > 0
    assert np.array_equal(film0.view(np.uint32), counted0.view(np.uint32))
    sc.attach_bsppaperinst(c.make(hprt, m))
    what = "%s, seed %d" % (name, seed)
    plain, st = sc.render()
    assert np.array_equal(plain.view(np.uint32), film0.view(np.uint32)), what
    counted, stc = sc.render(count_work=True)
    assert np.array_equal(counted.view(np.uint32), film0.view(np.uint32)), what + " (counting)"
    for k in ("camera_rays", "rays", "shadow_rays"):
        assert stc[k] == st0[k], (what, k, stc[k], st0[k])
    assert st["rays"] <= stc["rays"]
    stats_film, stp = sc.render(pixel_stats=True)
    assert np.array_equal(stats_film.view(np.uint32), film0.view(np.uint32)), what + " (pixel statistics)"
    s = sc.pixel_stats().reshape(-1, 7).sum(0)
    assert s[5] > 0 and s[6] > 0 and s[3] > 0
    assert s[5] == stp["nodes_entered"] and s[6] == stp["nodes_entered_p"]
    assert s[3] + s[5] == stp["nodes_fetched"] and s[4] + s[6] == stp["nodes_fetched_p"]
    assert s[1] == stp["tri_tests"] + stp["sphere_tests"] and s[2] == stp["tri_tests_p"] + stp["sphere_tests_p"]
    kdc = sc.kd_counters()
    if c.kd_aware:
        kd2 = sc.pixel_kd_stats()                                        # hprt_pixel_kd_stats_read
        assert (int(kd2[0].sum()), int(kd2[1].sum())) == kdc and kdc[0] > 0 and kdc[1] > 0
        px = sc.pixel_stats()
        assert (kd2[0] <= px[:, :, 5]).all() and (kd2[1] <= px[:, :, 6]).all()
    else:
        assert kdc == (0, 0) and not sc.pixel_kd_stats().any()


def test_four_two_level_attaches_in_turn_on_one_scene(hprt, orc, tmp_path):
    """KdInst, BspNodeInst fastkd, RbspInst, BspNodeInst plain on ONE scene, each held to its restatement; then a handle of another
    model is refused and the previous walk stays in place"""
    m, path = ks.bake(hprt, tmp_path, ks.scene_text(), "scene")
    kd, nk = hprt.KdInst(m), hprt.BspNodeInst(m, "bspclusterfastkd", n_directions=K, seed=SEED)
    rb, pl = hprt.RbspInst(m, kd_aware=False, n_directions=13), hprt.BspNodeInst(m, "bsprandom", n_directions=K, seed=SEED)
    kd_ref = kdinst_ref.KdInstScene(path).take(kd)
    nk_ref = bsppaperinst_ref.BspPaperInstScene(path, True).take(nk)
    rb_ref = rbspinst_ref.RbspInstScene(path, 13, False).take(rb)
    pl_ref = bsppaperinst_ref.BspPaperInstScene(path, False).take(pl)
    o, d, tm = _rays(m, pl_ref, orc.OracleScene(path), 256, 6)
    sc = hprt.Scene(m, hprt.Bvh(m), device=0)
    sc.attach_kdinst(kd)
    check_kd_parity(sc, kd_ref, o, d, tm)
    sc.attach_bsppaperinst(nk)
    check_parity(sc, nk_ref, o, d, tm)
    sc.attach_rbspinst(rb)
    check_parity(sc, rb_ref, o, d, tm)
    sc.attach_bsppaperinst(pl)
    check_parity(sc, pl_ref, o, d, tm)
    assert sc.kd_counters() == (0, 0)
    m2, _ = ns.bake(hprt, tmp_path, ns.only_instances_text("bsprandom"), "other")
    with pytest.raises(hprt.HprtError) as e:
        sc.attach_bsppaperinst(hprt.BspNodeInst(m2, "bsprandom", n_directions=K, seed=SEED))
    assert e.value.code == hprt.E_INVALID
    check_parity(sc, pl_ref, o, d, tm)


# ---- the device-assisted build ----

def _same_handles(a, b, objects):
    assert a.info() == b.info()
    for obj in [-1] + objects:
        ta, tb = (t.copy() if obj < 0 else t.object_copy(obj) for t in (a, b))
        assert ta[0].tobytes() == tb[0].tobytes() and ta[1].tobytes() == tb[1].tobytes(), obj
        assert a.bounds(obj).tobytes() == b.bounds(obj).tobytes()


@pytest.mark.parametrize("acc", ACCS)
def test_device_build_gives_the_hosts_bytes(hprt, own_scene, acc):
    """K = 4 on both scenes, every costed node through k_sweepcost (min_candidates = 1), one session for all trees of a handle"""
    for m, objects in ((own_scene[0], [ns.BLOB, ns.MIX]), (hprt.Model.load(ns.SIMPLE_INSTANCED), [0])):
        host = hprt.BspNodeInst(m, acc, n_directions=4)
        dev = hprt.BspNodeInst(m, acc, n_directions=4, device=0, min_candidates=1)
        _same_handles(dev, host, objects)
        st = dev.build_stats
        assert host.build_stats is None and st["nodes_device"] > 0 and st["candidates_device"] > 0 and st["candidates_recosted_on_host"] == 0, (acc, st)


def test_device_build_repairs_overflow_on_the_host(hprt, own_scene):
    """max_edges = 12, the root box's own edge count: an oblique cut's halves outgrow it, those candidates are costed again on the
    host, and the trees are the same"""
    m = own_scene[0]
    for acc in ("bsprandom", "bsprandomfastkd"):
        host = hprt.BspNodeInst(m, acc, n_directions=4)
        dev = hprt.BspNodeInst(m, acc, n_directions=4, device=0, min_candidates=1, max_edges=12)
        _same_handles(dev, host, [ns.BLOB, ns.MIX])
        st = dev.build_stats
        assert st["candidates_recosted_on_host"] > 0 and st["candidates_device"] > 0 and st["nodes_device"] > 0, (acc, st)
    with pytest.raises(hprt.HprtError) as e:
        hprt.BspNodeInst(m, "bsprandom", n_directions=4, device=0, max_edges=4096)      # may only lower the capacity
    assert e.value.code == hprt.E_INVALID


def test_a_refused_build_between_two_good_ones(hprt, own_scene):
    m = own_scene[0]
    host = hprt.BspNodeInst(m, "bspclusterwithkd", n_directions=4)
    _same_handles(hprt.BspNodeInst(m, "bspclusterwithkd", n_directions=4, device=0, min_candidates=1), host, [ns.BLOB, ns.MIX])
    with pytest.raises(hprt.HprtError) as e:
        hprt.BspNodeInst(m, "bspclusterwithkd", n_directions=2, device=0, min_candidates=1)
    assert e.value.code == hprt.E_UNSUPPORTED
    with pytest.raises(hprt.HprtError) as h:
        hprt.BspNodeInst(m, "bspclusterwithkd", n_directions=2)
    assert str(e.value) == str(h.value)                # the host entry's message
    _same_handles(hprt.BspNodeInst(m, "bspclusterwithkd", n_directions=4, device=0, min_candidates=1), host, [ns.BLOB, ns.MIX])
