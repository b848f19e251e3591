"""The two-level general BSP walks on the GPU (hprt_scene_attach_bsppaperinst, k_bsppaperinstwalk): closest and any hit held bit for
bit to the test-side restatement of BSP / BSPKd on both levels joined by TransformedPrimitive (tests/bsppaperinst_reference.cpp) —
t, primitive, instance, barycentrics, the four counters, the kd share — on a scene of our own, on degenerate rays and rays that
start on the split planes of an object's tree, on tests/golden/simple_instanced.hprt, on a scene of ties and on the deep pair of
staircases; a render against the BVH's film and the restatement's per-pixel sums; kernel resources; and, on one scene, four
two-level attaches in turn, for what they share.  Every case runs plain and kd-aware.  Nothing here has a tolerance."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
import bsppaperinst_ref
import bsppaperinst_scenes as bs
import deep_todo
import kdinst_ref
import kdinst_scenes as ks
import rbspinst_ref
import tree_ref
import tree_walk_checks as twc
from test_gpu_kdinst import check_parity as check_kd_parity
from test_gpu_rbspinst import _flags, _rays, check_parity      # (the two-level RBSP tests' checks read a restatement of this shape)

pytestmark = pytest.mark.gpu
SIMPLE_INSTANCED = os.path.join(GOLDEN, "simple_instanced.hprt")
CASES = [False, True]
IDS = ["bsppaper", "bsppaperkd"]
MAX_NAN_RAY_NODES = 200000


class _Case:
    def __init__(self, hprt, orc, m, path, kd, **kw):
        self.m, self.path, self.kd = m, path, kd
        self.trees = hprt.BspPaperInst(m, kd_aware=kd, **kw)
        self.sc = hprt.Scene(m, hprt.Bvh(m), device=0)
        self.sc.attach_bsppaperinst(self.trees)
        self.ref = bsppaperinst_ref.BspPaperInstScene(path, kd).take(self.trees)
        self.oracle = orc.OracleScene(path)

    def rays(self, n, seed):
        return _rays(self.m, self.ref, self.oracle, n, seed)


@pytest.fixture(scope="module", params=CASES, ids=IDS)
def own(request, hprt, orc, tmp_path_factory):
    kd = request.param
    m, path = bs.bake(hprt, tmp_path_factory.mktemp("bsppaperinst"), bs.scene_text(kd), "scene")
    return _Case(hprt, orc, m, path, kd)


def test_hits_equal_the_reference_walk_on_the_test_scene(own):
    o, d, tm = own.rays(20000, 1)
    assert np.isinf(tm).any() and np.isfinite(tm).any()
    t, p, inst = check_parity(own.sc, own.ref, o, d, tm)
    # every kind of entry is exercised: hits on top-level primitives, inside each of the eight instances (a tree under four
    # transforms, the identity among them, lone primitives, a tree with a sphere), and misses
    assert set(np.unique(inst).tolist()) == {-1} | set(range(bs.N_INSTANCES)) and (p < 0).any() and ((p >= 0) & (inst < 0)).any()


def _object_planes(trees, kd):
    """of the all-triangle object's tree: (axes [P, 3], splits [P]) of the nodes that take the dot-product step, and (axis number,
    split) of the kd nodes of a kd-aware tree"""
    nodes, _ = trees.object_copy(bs.BLOB)
    kind = nodes[:, 1] & (7 if kd else 1)
    dot = (kind == 4) if kd else (kind == 0)
    kdn = (kind < 3) if kd else np.zeros(kind.shape, bool)
    return (nodes[dot, 2:5].copy().view(np.float32), nodes[dot, 0].copy().view(np.float32), kind[kdn].astype(np.int64), nodes[kdn, 0].copy().view(np.float32))


def _on_plane_rays(own, n, rng):
    """Rays in the object space of the all-triangle object, which is world space for its instance under the identity.  Plane
    family: origins with float Dot(axis, o) == split of one of the tree's dot-product nodes and a direction with Dot(axis, d) == 0
    exactly — (ay, -ax, 0), (az, 0, -ax) or (0, az, -ay) times a power of two: the two products cancel bit for bit.  kd family
    (kd-aware trees): o[axis] == split of one of its kd nodes with d[axis] = +-0, where the kd form reads the side from d[axis]
    and the dot-product form from 1 / Dot = +-inf."""
    b = own.ref.tree_bounds(bs.BLOB)
    blo, ext = b[:3], b[3:] - b[:3]
    axes, pos, kd_axis, kd_pos = _object_planes(own.trees, own.kd)
    assert axes.shape[0] > 0 and (np.count_nonzero(axes, axis=1) > 1).any()
    out = []
    pick = rng.integers(0, pos.shape[0], 3 * n)
    a, s = axes[pick], pos[pick]
    o = (blo + rng.uniform(0, 1, (3 * n, 3)) * ext).astype(np.float32)
    o, ok = twc._on_plane(a, s, o)
    z = np.zeros(3 * n, np.float32)
    forms = np.stack([np.stack([a[:, 1], -a[:, 0], z], 1), np.stack([a[:, 2], z, -a[:, 0]], 1), np.stack([z, a[:, 2], -a[:, 1]], 1)])
    d = forms[rng.integers(0, 3, 3 * n), np.arange(3 * n)] * np.ldexp(np.where(rng.uniform(size=3 * n) < 0.5, -1.0, 1.0), rng.integers(-3, 4, 3 * n)).astype(np.float32)[:, None]
    d = d.astype(np.float32)
    ok &= d.any(1) & (twc._dot32(a, d) == 0)
    assert ok.sum() >= n, int(ok.sum())
    keep = np.nonzero(ok)[0][:n]
    out.append((o[keep], d[keep], np.full(n, np.inf, np.float32)))
    if own.kd:
        assert kd_axis.shape[0] > 0
        pick = rng.integers(0, kd_axis.shape[0], n)
        ax, sp = kd_axis[pick], kd_pos[pick]
        rows = np.arange(n)
        o = (blo + rng.uniform(0, 1, (n, 3)) * ext).astype(np.float32)
        o[rows, ax] = sp
        d = rng.normal(size=(n, 3)).astype(np.float32)
        d[rows, ax] = np.where(rng.uniform(size=n) < 0.5, np.float32(0.0), np.float32(-0.0))
        out.append((o, d, np.full(n, np.inf, np.float32)))
    return out


def test_degenerate_and_on_plane_rays(own):
    rng = np.random.default_rng(11)
    b = own.ref.tree_bounds()
    families = [twc.degenerate_rays(rng, b[:3], b[3:] - b[:3], 4096)] + _on_plane_rays(own, 2048, rng)
    assert np.isnan(families[0][1]).all(1).any()
    kd_forms_differ = False
    for o, d, tm in families:
        c0 = own.ref.intersect(o, d, tm)[4]
        k0 = own.ref.occluded(o, d, tm)[1]
        # (a ray with a NaN direction enters every object tree it meets: the scene is small enough for a lane of the device walk)
        assert max(int(c0[:, 0].max()), int(k0[:, 0].max())) < MAX_NAN_RAY_NODES
        t, p, inst = check_parity(own.sc, own.ref, o, d, tm)
        if own.kd:
            own.ref.dot_only(True)
            try:
                r2 = own.ref.intersect(o, d, tm)
                q2 = own.ref.occluded(o, d, tm)
            finally:
                own.ref.dot_only(False)
            kd_forms_differ |= bool(((r2[4] != c0).any(1) | (r2[1] != p) | (twc._bits(r2[0]) != twc._bits(t)) | (q2[1] != k0).any(1)).any())
    # the instance under the identity is reached by the families built in its object space
    assert (inst == bs.IDENTITY_INSTANCE).any()
    if own.kd:
        assert kd_forms_differ, "no ray tells the kd form from the dot-product form: the family tests nothing"


def test_device_entry_points_walk_the_two_level_trees(own):
    twc.check_device_entry_points(own.sc, *own.rays(2048, 2))


@pytest.mark.parametrize("kd", CASES, ids=IDS)
def test_hits_equal_the_reference_walk_on_simple_instanced(hprt, orc, kd):
    """the golden scene whose top level holds only the instance (a baked model carries no Accelerator line: the defaults as keywords)"""
    case = _Case(hprt, orc, hprt.Model.load(SIMPLE_INSTANCED), SIMPLE_INSTANCED, kd, isect_cost=80)
    _, p, inst = check_parity(case.sc, case.ref, *case.rays(20000, 3))
    assert (inst >= 0).any() and (p < 0).any()


@pytest.mark.parametrize("kd", CASES, ids=IDS)
def test_a_tie_between_two_instances_goes_the_reference_walks_way(hprt, orc, tmp_path, kd):
    """every triangle of one instance coincides with a triangle of another: the walk returns the restatement's choice for every ray,
    whichever it is"""
    m, path = bs.bake(hprt, tmp_path, bs.tie_text(kd), "tie")
    case = _Case(hprt, orc, m, path, kd)
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
    assert s[1] == stc["tri_tests"] + stc["sphere_tests"] and s[2] == stc["tri_tests_p"] + stc["sphere_tests_p"]
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


@pytest.mark.parametrize("kd", CASES, ids=IDS)
def test_the_one_list_past_its_lds_entries_up_to_capacity(hprt, orc, tmp_path, kd):
    """the deep pair (tests/bsppaperinst_scenes.py): top-level entries, the saved position and the object's entries together cross
    the eight LDS entries and reach the 64 the attach rule allows.  One level more never reaches a scene: set_tree refuses it, the
    handle keeps the accepted pair, and the scene the pair is attached to keeps walking it."""
    pair = bs.DeepPair(kd)
    m, path = bs.bake(hprt, tmp_path, pair.text(), "deep")
    trees, ref = hprt.BspPaperInst(m, kd_aware=kd), bsppaperinst_ref.BspPaperInstScene(path, kd)
    pair.install(trees, ref)
    sc = hprt.Scene(m, hprt.Bvh(m), device=0)
    sc.attach_bsppaperinst(trees)
    o, d, tm = pair.deep_rays(8192)
    todo = ref.intersect(o, d, tm)[5]
    assert (todo[::2] == deep_todo.CAPACITY).all() and (todo <= 8).any() and (todo == 9).any()
    t, p, inst = check_parity(sc, ref, o, d, tm)
    assert (inst == 0).any() and ((p >= 0) & (inst < 0)).any()
    # the BVH knows these hits too: the staircases have no ties
    t2, p2, i2, _ = hprt.Scene(m, hprt.Bvh(m), device=0).intersect_instanced(o, d, tm)
    assert np.array_equal(p, p2) and np.array_equal(inst, i2) and np.array_equal(twc._bits(t), twc._bits(t2))
    # 5 + 59 + 1: a model whose object has one level more.  Its handle never holds the pair (set_tree: HPRT_E_UNSUPPORTED), and the
    # handle as it stands belongs to another model: the attach refuses it and the 64-entry walk stays in place
    deeper = bs.DeepPair(kd, bs.OBJECT_LEVELS + 1)
    m2, path2 = bs.bake(hprt, tmp_path, deeper.text(), "deeper")
    trees2, ref2 = hprt.BspPaperInst(m2, kd_aware=kd), bsppaperinst_ref.BspPaperInstScene(path2, kd)
    trees2.set_tree(-1, *deeper.trees()[-1], ref2.tree_bounds(-1))
    with pytest.raises(hprt.HprtError) as e:
        trees2.set_tree(0, *deeper.trees()[0], ref2.tree_bounds(0))
    assert e.value.code == hprt.E_UNSUPPORTED
    with pytest.raises(hprt.HprtError) as e:
        sc.attach_bsppaperinst(trees2)
    assert e.value.code == hprt.E_INVALID
    check_parity(sc, ref, o[:512], d[:512], tm[:512])


def test_attach_refusals(hprt, own, tmp_path):
    m2, _ = bs.bake(hprt, tmp_path, bs.tie_text(own.kd), "tie")
    with pytest.raises(hprt.HprtError) as e:
        own.sc.attach_bsppaperinst(hprt.BspPaperInst(m2, kd_aware=own.kd))                    # another model's trees
    assert e.value.code == hprt.E_INVALID
    o, d, tm = own.rays(256, 5)
    check_parity(own.sc, own.ref, o, d, tm)                      # the refused attach left the walk in place
    # the single-level attaches answer an instanced scene what they answered before, and leave the walk in place too
    single = (hprt.BspPaperKd if own.kd else hprt.BspPaper).from_triangles(bs.blob_triangles())
    with pytest.raises(hprt.HprtError) as e:
        getattr(own.sc, "attach_bsppaperkd" if own.kd else "attach_bsppaper")(single)
    assert e.value.code == hprt.E_UNSUPPORTED and "trees over object instances are not supported: the scene keeps its BVH" in str(e.value)
    check_parity(own.sc, own.ref, o, d, tm)
    plain, _ = bs.bake(hprt, tmp_path, bs.no_instances(own.kd), "plain")
    with pytest.raises(hprt.HprtError) as e:
        hprt.Scene(plain, hprt.Bvh(plain), device=0).attach_bsppaperinst(own.trees)
    assert e.value.code == hprt.E_UNSUPPORTED


def test_four_two_level_attaches_in_turn_on_one_scene(hprt, orc, tmp_path):
    """What the attaches share — the node, primitive, entry and axis buffers, the kd counter pair, the reset descriptors — across
    changes of walk: on ONE scene (tests/kdinst_scenes.py's) the two-level kd-trees, kd-aware general BSP trees, RBSP trees of 13
    directions and plain general BSP trees, each held to its restatement bit for bit; and a single-level bsppaper attach on a scene
    without instances still works afterwards."""
    m, path = ks.bake(hprt, tmp_path, ks.scene_text(), "scene")
    kd, bk = hprt.KdInst(m), hprt.BspPaperInst(m, kd_aware=True, isect_cost=80)
    rb, bp = hprt.RbspInst(m, kd_aware=False, n_directions=13), hprt.BspPaperInst(m, kd_aware=False, isect_cost=80)
    kd_ref = kdinst_ref.KdInstScene(path).take(kd)
    bk_ref = bsppaperinst_ref.BspPaperInstScene(path, True).take(bk)
    rb_ref = rbspinst_ref.RbspInstScene(path, 13, False).take(rb)
    bp_ref = bsppaperinst_ref.BspPaperInstScene(path, False).take(bp)
    o, d, tm = _rays(m, bp_ref, orc.OracleScene(path), 256, 6)
    sc = hprt.Scene(m, hprt.Bvh(m), device=0)
    sc.attach_kdinst(kd)
    check_kd_parity(sc, kd_ref, o, d, tm)
    sc.attach_bsppaperinst(bk)
    check_parity(sc, bk_ref, o, d, tm)
    sc.attach_rbspinst(rb)
    check_parity(sc, rb_ref, o, d, tm)
    sc.attach_bsppaperinst(bp)
    check_parity(sc, bp_ref, o, d, tm)
    assert sc.kd_counters() == (0, 0)
    m2, path2 = bs.bake(hprt, tmp_path, bs.no_instances(False), "plain")
    tree = hprt.BspPaper(m2)
    sc2 = hprt.Scene(m2, hprt.Bvh(m2), device=0)
    sc2.attach_bsppaper(tree)
    ref2 = tree_ref.BspScene(path2, build=False)
    ref2.set_tree(*tree.arrays())
    rng = np.random.default_rng(7)                               # the scene is a floor: rays from above it, most of them downwards
    o2 = np.concatenate([rng.uniform(-3.5, 3.5, (512, 2)), rng.uniform(0.5, 1.5, (512, 1))], 1).astype(np.float32)
    d2 = np.concatenate([rng.normal(size=(512, 2)), -np.abs(rng.normal(size=(512, 1)))], 1).astype(np.float32)
    d2[::8, 2] *= -1
    tm2 = np.where(rng.uniform(size=512) < 0.5, np.inf, rng.uniform(0, 4, 512)).astype(np.float32)
    t0, p0, b0, c0 = ref2.intersect(o2, d2, tm2)
    t1, p1, b1, c1 = sc2.intersect(o2, d2, tm2, count=True)
    assert np.array_equal(p0, p1) and np.array_equal(twc._bits(t0), twc._bits(t1)) and np.array_equal(twc._bits(b0), twc._bits(b1))
    assert c1.tolist() == c0[:, :4].sum(0).tolist() and (p0 >= 0).any()
    twc.check_any(sc2, ref2, [(o2, d2, tm2)])
    check_parity(sc, bp_ref, o, d, tm)                           # and the instanced scene still walks its trees


def test_bsppaperinst_walk_resources(tmp_path):
    """The sixteen variants <ANY_HIT, COUNT, QUAD, KD>: eight 8-byte todo entries per lane of a 256-thread workgroup in LDS and
    nothing else (no direction table); nothing spilled; the triangle-only ones within the 128 registers of the four workgroups per
    CU they are launched with and without a byte of scratch, the quadric ones within the 168 of three, their only private memory
    the frame of the interval-arithmetic sphere test's call — the bytes k_bsppaperwalk's quadric variants have for it."""
    meta = twc.kernel_metadata(twc.LIBHPRT, tmp_path)
    ks16 = {n: k for n, k in meta.items() if "k_bsppaperinstwalk" in n}
    single_quad = {k[".private_segment_fixed_size"] for n, k in meta.items() if "k_bsppaperwalkI" in n and _flags(n, "k_bsppaperwalk")[2]}
    assert len(ks16) == 16 and len(single_quad) == 1, (sorted(ks16), single_quad)
    assert len({tuple(_flags(n, "k_bsppaperinstwalk")[:4]) for n in ks16}) == 16
    for name, k in ks16.items():
        quad = _flags(name, "k_bsppaperinstwalk")[2]
        assert k[".group_segment_fixed_size"] == 8 * 256 * 8, name
        assert k[".vgpr_spill_count"] == 0 and k[".vgpr_count"] <= (168 if quad else 128), (name, k[".vgpr_count"])
        assert k[".private_segment_fixed_size"] == (next(iter(single_quad)) if quad else 0), (name, k[".private_segment_fixed_size"])
