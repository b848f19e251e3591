"""The two-level RBSP walks on the GPU (hprt_scene_attach_rbspinst, k_rbspinstwalk): closest and any hit held bit for bit to the
test-side restatement of RBSP / RBSPKd on both levels joined by TransformedPrimitive (tests/rbspinst_reference.cpp) — t, primitive,
instance, barycentrics, the four counters, the kd share — on a scene of our own, on tests/golden/simple_instanced.hprt, on a scene
of ties and on the deep pair of staircases; a render against the BVH's film and the restatement's per-pixel sums; kernel resources;
and, on one scene, the two-level kd-trees, RBSP trees and kd-trees again, for what the two attaches share.
Every case runs plain at M = 13 and kd-aware at M = 9."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
import deep_todo
import kdinst_ref
import kdinst_scenes as ks
import rbspinst_ref
import rbspinst_scenes as rs
import tree_walk_checks as twc
from test_gpu_kdinst import check_parity as check_kd_parity

pytestmark = pytest.mark.gpu
SIMPLE_INSTANCED = os.path.join(GOLDEN, "simple_instanced.hprt")
CASES = [(False, 13), (True, 9)]
IDS = ["rbsp13", "rbspkd9"]


class _Case:
    def __init__(self, hprt, orc, m, path, kd, M, n_directions=None):
        self.m, self.path, self.kd, self.M = m, path, kd, M
        self.trees = hprt.RbspInst(m, kd_aware=kd, n_directions=n_directions)
        self.sc = hprt.Scene(m, hprt.Bvh(m), device=0)
        self.sc.attach_rbspinst(self.trees)
        self.ref = rbspinst_ref.RbspInstScene(path, M, kd).take(self.trees)
        self.oracle = orc.OracleScene(path)

    def rays(self, n, seed):
        return _rays(self.m, self.ref, self.oracle, n, seed)


def _rays(m, ref, oracle, n, seed):
    """n camera rays and n random rays from inside and around the top-level bounds, finite and infinite (test_gpu_kdinst._Case.rays)"""
    rng = np.random.default_rng(seed)
    b = ref.tree_bounds()
    blo, ext = b[:3], b[3:] - b[:3]
    x0, y0, x1, y1 = m.options.film_bounds()
    oc, dc = oracle.camera_rays(rng.integers(x0, x1, n).astype(np.int32), rng.integers(y0, y1, n).astype(np.int32), rng.integers(0, 2, n).astype(np.int64))
    o, d, tm = twc.random_rays(rng, blo, ext, n)
    return np.concatenate([oc, o]).astype(np.float32), np.concatenate([dc, d]).astype(np.float32), np.concatenate([np.full(n, np.inf, np.float32), tm])


def check_parity(sc, ref, o, d, tm):
    """hprt_intersect_instanced, hprt_intersect and hprt_occluded against the restatement, with counting on — the four counters and
    the kd share (zero for plain trees); returns the restatement's closest hits"""
    t0, p0, i0, b0, c0, _ = ref.intersect(o, d, tm)
    t1, p1, i1, b1, c1 = sc.intersect_instanced(o, d, tm, count=True)
    assert np.array_equal(p0, p1), int((p0 != p1).sum())
    assert np.array_equal(i0, i1), int((i0 != i1).sum())
    assert np.array_equal(twc._bits(t0), twc._bits(t1)) and np.array_equal(twc._bits(b0), twc._bits(b1))
    s = c0.sum(0)
    assert c1.tolist() == [int(s[0]), int(s[1]), int(s[3]), int(s[4])], (c1, s)
    assert sc.kd_counters() == (int(s[5]), 0), (sc.kd_counters(), s)
    assert ref.kd_aware == (s[5] > 0)
    t2, p2, b2 = sc.intersect(o, d, tm)          # the entry point without the instance: the same walk
    assert np.array_equal(p2, p1) and np.array_equal(twc._bits(t2), twc._bits(t1))
    occ0, k0, _ = ref.occluded(o, d, tm)
    occ1, k1 = sc.occluded(o, d, tm, count=True)
    assert np.array_equal(occ0, occ1), int((occ0 != occ1).sum())
    s = k0.sum(0)
    assert k1.tolist() == [int(s[0]), int(s[1]), int(s[3]), int(s[4])], (k1, s)
    assert sc.kd_counters() == (0, int(s[5])), (sc.kd_counters(), s)
    return t0, p0, i0


@pytest.fixture(scope="module", params=CASES, ids=IDS)
def own(request, hprt, orc, tmp_path_factory):
    kd, M = request.param
    m, path = rs.bake(hprt, tmp_path_factory.mktemp("rbspinst"), rs.scene_text(kd, M), "scene")
    return _Case(hprt, orc, m, path, kd, M)


def test_hits_equal_the_reference_walk_on_the_test_scene(own):
    o, d, tm = own.rays(20000, 1)
    t, p, inst = check_parity(own.sc, own.ref, o, d, tm)
    # every kind of entry is exercised: hits on top-level primitives, inside each of the six instances (a tree, a lone primitive, a
    # tree with a sphere), and misses
    assert set(np.unique(inst).tolist()) == {-1, 0, 1, 2, 3, 4, 5} and (p < 0).any() and ((p >= 0) & (inst < 0)).any()


def test_device_entry_points_walk_the_two_level_trees(own):
    twc.check_device_entry_points(own.sc, *own.rays(2048, 2))


@pytest.mark.parametrize("kd,M", CASES, ids=IDS)
def test_hits_equal_the_reference_walk_on_simple_instanced(hprt, orc, kd, M):
    """the golden scene whose top level holds only the instance (a baked model carries no Accelerator line: M comes as a keyword)"""
    case = _Case(hprt, orc, hprt.Model.load(SIMPLE_INSTANCED), SIMPLE_INSTANCED, kd, M, n_directions=M)
    _, p, inst = check_parity(case.sc, case.ref, *case.rays(20000, 3))
    assert (inst >= 0).any() and (p < 0).any()


@pytest.mark.parametrize("kd,M", CASES, ids=IDS)
def test_a_tie_between_two_instances_goes_the_reference_walks_way(hprt, orc, tmp_path, kd, M):
    """every triangle of one instance coincides with a triangle of another: the walk returns the restatement's choice for every ray,
    whichever it is"""
    m, path = rs.bake(hprt, tmp_path, rs.tie_text(kd, M), "tie")
    case = _Case(hprt, orc, m, path, kd, M)
    o, d, tm = case.rays(10000, 4)
    t, p, inst = check_parity(case.sc, case.ref, o, d, tm)
    assert (inst >= 0).mean() >= 0.01          # the twins cover a few percent of the image: at least one ray in a hundred ends on one
    # and they are ties: the BVH walk may choose differently, but at the same t
    bvh = hprt.Scene(m, hprt.Bvh(m), device=0)
    t2, p2, i2, _ = bvh.intersect_instanced(o, d, tm)
    assert np.array_equal(twc._bits(t), twc._bits(t2))


def test_render_equals_the_bvh_film_and_pixel_statistics_the_reference_sums(hprt, own):
    m, sc, ref, oracle = own.m, own.sc, own.ref, own.oracle
    opt = m.options.copy()
    assert (opt.xres, opt.yres, opt.spp, opt.max_depth) == (64, 48, 2, 3)
    film, st = sc.render(opt)
    bvh_film, _ = hprt.Scene(m, hprt.Bvh(m), device=0).render(opt)
    assert np.array_equal(film.view(np.uint32), bvh_film.view(np.uint32))
    assert np.isfinite(film).all() and film[..., :3].max() > 0
    counted, stc = sc.render(opt, count_work=True, pixel_stats=True)
    px = sc.pixel_stats()
    s = px.reshape(-1, 7).sum(0)
    assert s[5] == stc["nodes_entered"] and s[6] == stc["nodes_entered_p"] and s[6] > 0
    assert s[3] + s[5] == stc["nodes_fetched"] and s[4] + s[6] == stc["nodes_fetched_p"]
    kdc = sc.kd_counters()
    if own.kd:
        kd2 = sc.pixel_kd_stats()
        assert int(kd2[0].sum()) == kdc[0] > 0 and int(kd2[1].sum()) == kdc[1] > 0
        assert (kd2[0] <= px[:, :, 5]).all() and (kd2[1] <= px[:, :, 6]).all()
    else:
        assert kdc == (0, 0) and not sc.pixel_kd_stats().any()      # plain trees: no node is a kd node
    # maxdepth 0 traces the camera rays and nothing else (the path ends before its first light sample): each pixel's statistics
    # are the restatement's counters summed over that pixel's camera rays
    opt0 = m.options.copy()
    opt0.max_depth = 0
    _, st0 = sc.render(opt0, count_work=True, pixel_stats=True)
    px = sc.pixel_stats()
    x0, y0, x1, y1 = opt0.film_bounds()
    H, W, spp = y1 - y0, x1 - x0, opt0.spp
    yy, xx = np.mgrid[y0:y1, x0:x1]
    want = np.zeros((H, W, 4), np.uint64)
    for smp in range(spp):
        o, d = oracle.camera_rays(xx.ravel().astype(np.int32), yy.ravel().astype(np.int32), np.full(H * W, smp, np.int64))
        c = ref.intersect(o, d, np.full(H * W, np.inf, np.float32))[4]
        want += np.stack([c[:, 3] + c[:, 4], c[:, 2], c[:, 1], c[:, 5]], 1).reshape(H, W, 4)
    assert st0["rays"] == H * W * spp and st0["shadow_rays"] == 0
    assert np.array_equal(px[:, :, 1], want[:, :, 0]) and np.array_equal(px[:, :, 3], want[:, :, 1]) and np.array_equal(px[:, :, 5], want[:, :, 2])
    assert not px[:, :, [2, 4, 6]].any()
    if own.kd:
        kd2 = sc.pixel_kd_stats()
        assert np.array_equal(kd2[0].reshape(H, W), want[:, :, 3]) and want[:, :, 3].sum() > 0 and not kd2[1].any()
    else:
        assert not want[:, :, 3].any() and sc.kd_counters() == (0, 0) and not sc.pixel_kd_stats().any()


@pytest.mark.parametrize("kd", [False, True], ids=["rbsp7", "rbspkd9"])
def test_the_one_list_past_its_lds_entries_up_to_capacity(hprt, orc, tmp_path, kd):
    """the deep pair (tests/rbspinst_scenes.py): top-level entries, the saved position and the object's entries together cross the
    eight LDS entries and reach the 64 the attach rule allows (hand-made staircases: M = 7 plain, 9 kd-aware, as tests/deep_todo.py
    encodes them)"""
    pair = rs.DeepPair(kd)
    m, path = rs.bake(hprt, tmp_path, pair.text(), "deep")
    trees, ref = hprt.RbspInst(m, kd_aware=kd), rbspinst_ref.RbspInstScene(path, pair.M, kd)
    pair.install(trees, ref)
    sc = hprt.Scene(m, hprt.Bvh(m), device=0)
    sc.attach_rbspinst(trees)
    o, d, tm = pair.deep_rays(8192)
    todo = ref.intersect(o, d, tm)[5]
    assert (todo[::2] == deep_todo.CAPACITY).all() and (todo <= 8).any() and (todo == 9).any()
    t, p, inst = check_parity(sc, ref, o, d, tm)
    assert (inst == 0).any() and ((p >= 0) & (inst < 0)).any()
    # the BVH knows these hits too: the staircases have no ties
    t2, p2, i2, _ = hprt.Scene(m, hprt.Bvh(m), device=0).intersect_instanced(o, d, tm)
    assert np.array_equal(p, p2) and np.array_equal(inst, i2) and np.array_equal(twc._bits(t), twc._bits(t2))


def test_attach_refusals(hprt, own, tmp_path):
    m2, _ = rs.bake(hprt, tmp_path, rs.tie_text(own.kd, own.M), "tie")
    with pytest.raises(hprt.HprtError) as e:
        own.sc.attach_rbspinst(hprt.RbspInst(m2, kd_aware=own.kd))                    # another model's trees
    assert e.value.code == hprt.E_INVALID
    o, d, tm = own.rays(256, 5)
    check_parity(own.sc, own.ref, o, d, tm)                      # the refused attach left the walk in place
    plain, _ = rs.bake(hprt, tmp_path, rs.no_instances(own.kd, own.M), "plain")
    with pytest.raises(hprt.HprtError) as e:
        hprt.Scene(plain, hprt.Bvh(plain), device=0).attach_rbspinst(own.trees)
    assert e.value.code == hprt.E_UNSUPPORTED


def test_kd_then_rbspkd_then_kd_trees_on_one_scene(hprt, orc, tmp_path):
    """What the two attaches share — the entry buffer, the kd counter pair, the reset descriptor — across a change of walk: on ONE
    scene (tests/kdinst_scenes.py's) the two-level kd-trees, then kd-aware two-level RBSP trees over the same model, then the
    kd-trees again, each held to its restatement bit for bit"""
    m, path = ks.bake(hprt, tmp_path, ks.scene_text(), "scene")
    kd, rb = hprt.KdInst(m), hprt.RbspInst(m, kd_aware=True, n_directions=9)
    kd_ref = kdinst_ref.KdInstScene(path).take(kd)
    rb_ref = rbspinst_ref.RbspInstScene(path, 9, True).take(rb)
    o, d, tm = _rays(m, rb_ref, orc.OracleScene(path), 256, 6)
    sc = hprt.Scene(m, hprt.Bvh(m), device=0)
    sc.attach_kdinst(kd)
    check_kd_parity(sc, kd_ref, o, d, tm)
    sc.attach_rbspinst(rb)
    check_parity(sc, rb_ref, o, d, tm)
    sc.attach_kdinst(kd)
    check_kd_parity(sc, kd_ref, o, d, tm)
    assert sc.kd_counters() == (0, 0)


def _flags(name, kernel):
    """the template arguments <..., Lb?E> of a mangled kernel name as a list of bools"""
    return [x.startswith("1") for x in name.split(kernel + "I")[1].split("Lb")[1:]]


def test_rbspinst_walk_resources(tmp_path):
    """The sixteen variants <ANY_HIT, COUNT, QUAD, KD>: eight 8-byte todo entries per lane of a 256-thread workgroup and the
    direction table (3 * 13 floats) in LDS; nothing spilled; the triangle-only ones within the 128 registers of the four workgroups
    per CU they are launched with and without a byte of scratch, the quadric ones within the 168 of three, their only private memory
    the frame of the interval-arithmetic sphere test's call — the bytes k_rbspwalk's quadric variants have for it."""
    meta = twc.kernel_metadata(twc.LIBHPRT, tmp_path)
    ks16 = {n: k for n, k in meta.items() if "k_rbspinstwalk" in n}
    rbsp_quad = {k[".private_segment_fixed_size"] for n, k in meta.items() if "k_rbspwalkI" in n and _flags(n, "k_rbspwalk")[2]}
    assert len(ks16) == 16 and len(rbsp_quad) == 1, (sorted(ks16), rbsp_quad)
    assert len({tuple(_flags(n, "k_rbspinstwalk")[:4]) for n in ks16}) == 16
    for name, k in ks16.items():
        quad = _flags(name, "k_rbspinstwalk")[2]
        assert k[".group_segment_fixed_size"] == 8 * 256 * 8 + 4 * 3 * 13, name
        assert k[".vgpr_spill_count"] == 0 and k[".vgpr_count"] <= (168 if quad else 128), (name, k[".vgpr_count"])
        assert k[".private_segment_fixed_size"] == (next(iter(rbsp_quad)) if quad else 0), (name, k[".private_segment_fixed_size"])
