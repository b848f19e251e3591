"""The rbspkd walk on the GPU (Accelerator "rbspkd"): closest and any hit held bit for bit to the test-side restatement of
RBSPKd::Intersect / IntersectP (tests/rbspkd_reference.cpp) — t, primitive, barycentrics, all four counters and the kd share — on
camera, random, degenerate, infinite and on-a-split-plane rays, including rays built so that the kd form of an axis node and
RBSP's dot-product form disagree; renders against the reference's images; per-pixel kd statistics; tile sharding; switching
between the kd, RBSP and rbspkd walks; attach refusals; kernel resources."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, KILLEROO, ROOT
import rbspkd_ref

pytestmark = pytest.mark.gpu
DODECA = os.path.join(GOLDEN, "dodecahedron.hprt")
CASES = [(DODECA, 3), (DODECA, 7), (DODECA, 9), (DODECA, 13), (KILLEROO, 3), (KILLEROO, 7)]


@pytest.fixture(scope="module", params=CASES, ids=["dodecahedron-3", "dodecahedron-7", "dodecahedron-9", "dodecahedron-13", "killeroo-simple-3",
                                                   "killeroo-simple-7"])
def rk(request, hprt, orc):
    path, M = request.param
    m = hprt.Model.load(path)
    bvh = hprt.Bvh(m)
    sc = hprt.Scene(m, bvh, device=0)
    tree = hprt.RbspKd(m, n_directions=M)
    sc.attach_rbspkd(tree)
    if path == DODECA:
        ref = rbspkd_ref.RbspKdScene(path, M)                 # the restated build: the library's tree must be the same
        nodes, idx = tree.arrays()
        rn, ri = ref.tree()
        assert np.array_equal(nodes, rn) and np.array_equal(idx, ri)
    else:
        ref = rbspkd_ref.RbspKdScene(path, M, build=False)   # killeroo-simple's restated build is slow: walk the library's tree
        ref.set_tree(*tree.arrays())
    b = np.array(bvh.info()["bounds"], np.float32)
    return path, M, m, sc, tree, ref, orc.OracleScene(path), (b[:3], b[3:])


def _dot32(d, o):
    """Dot(direction, o) in float32, x*x + y*y + z*z left to right (one rounding per operation)"""
    d = d.astype(np.float32); o = o.astype(np.float32)
    return ((d[..., 0] * o[..., 0] + d[..., 1] * o[..., 1]) + d[..., 2] * o[..., 2]).astype(np.float32)


def _on_plane(dirs, ax, pos, o):
    """Move each origin onto its split plane so that the float Dot(dir, o) equals the split exactly: project, then step the
    coordinate with the largest direction component by nextafter.  Returns the origins and which of them made it."""
    d = dirs[ax].astype(np.float64)
    o = (o + (pos.astype(np.float64) - (o.astype(np.float64) * d).sum(1))[:, None] * d).astype(np.float32)
    k = np.abs(dirs[ax]).argmax(1)
    rows = np.arange(o.shape[0])
    for _ in range(200):
        v = _dot32(dirs[ax], o)
        bad = v != pos
        if not bad.any():
            break
        up = (v < pos) == (dirs[ax][rows, k] > 0)
        cur = o[rows, k]
        o[rows, k] = np.where(bad, np.nextafter(cur, np.where(up, np.float32(np.inf), np.float32(-np.inf))).astype(np.float32), cur)
    return o, _dot32(dirs[ax], o) == pos


def _bits(a):
    """float bits with every NaN made one (the host's and the device's NaNs carry different sign / payload bits)"""
    a = np.where(np.isnan(a), np.float32(np.nan), a).astype(np.float32)
    return a.view(np.uint32)


def _srgb8(rgb):
    v = rgb.astype(np.float64)
    g = np.where(v <= 0.0031308, 12.92 * v, 1.055 * np.power(np.maximum(v, 1e-30), 1 / 2.4) - 0.055)
    return np.clip(255.0 * g + 0.5, 0, 255).astype(np.int32)


def _splits(tree):
    """(direction, split position) of every interior node of the tree"""
    nodes, _ = tree.arrays()
    M = tree.info()["M"]
    mask = (1 << M.bit_length()) - 1
    ax = nodes[:, 1] & mask
    inner = ax != M
    return ax[inner].astype(np.int64), nodes[inner, 0].view(np.float32)


def _rays(tree, ref, oracle, bounds, n, seed):
    rng = np.random.default_rng(seed)
    blo, bhi = bounds
    ext = bhi - blo
    out = []
    # camera rays
    o, d = oracle.camera_rays(rng.integers(0, 700, n).astype(np.int32), rng.integers(0, 700, n).astype(np.int32), rng.integers(0, 8, n).astype(np.int64))
    out.append((o, d, np.full(n, np.inf, np.float32)))
    # random rays from inside and around the scene, finite and infinite
    o = (blo + rng.uniform(-0.2, 1.2, (n, 3)) * ext).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    tm = np.where(rng.uniform(size=n) < 0.5, np.inf, rng.uniform(0, 1, n) * np.linalg.norm(ext)).astype(np.float32)
    out.append((o, d, tm))
    # zero direction components of either sign, -0 origins, NaN / +-inf directions and origins
    o = (blo + rng.uniform(-0.2, 1.2, (n, 3)) * ext).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    k = n // 10
    d[:k, 0] = 0.0; d[k:2 * k, 1] = -0.0; d[2 * k:3 * k, 0] = -0.0; d[2 * k:3 * k, 2] = 0.0
    d[3 * k:4 * k, 0] = -0.0; d[3 * k:4 * k, 1:] = np.abs(d[3 * k:4 * k, 1:])
    o[3 * k:4 * k, 0] = -0.0
    d[4 * k:4 * k + 8] = np.nan; d[4 * k + 8:4 * k + 16, 1] = np.inf; d[4 * k + 16:4 * k + 24, 2] = -np.inf
    o[4 * k + 24:4 * k + 32, 0] = np.inf
    out.append((o, d, np.full(n, np.inf, np.float32)))
    # origins exactly on split planes, oblique ones included (float Dot(dir, o) == split), with direction components zeroed
    ax, pos = _splits(tree)
    dirs = tree.directions()
    pick = rng.integers(0, ax.shape[0], n)
    o = (blo + rng.uniform(0, 1, (n, 3)) * ext).astype(np.float32)
    o, ok = _on_plane(dirs, ax[pick], pos[pick], o)
    assert ok.mean() > 0.5, ok.mean()
    d = rng.normal(size=(n, 3)).astype(np.float32)
    third = n // 3
    d[:third] = np.where(dirs[ax[pick][:third]] != 0, np.float32(0.0), d[:third])
    d[third:2 * third, rng.integers(0, 3)] = -0.0
    out.append((o[ok], d[ok], np.full(int(ok.sum()), np.inf, np.float32)))
    out.append(_separating_rays(tree, bounds, n, rng))
    return out


def _separating_rays(tree, bounds, n, rng):
    """Rays on which the kd form of an axis node and the dot-product form disagree: origins exactly on the tree's own axis
    splits with d[axis] = +-0 (kd: belowFirst; dot: 1 / (+0) = +inf, not below first) or +-inf, and origins with a +-inf or -0
    component off the axis (the dot product turns 0 * inf into NaN)."""
    blo, bhi = bounds
    ext = bhi - blo
    ax, pos = _splits(tree)
    kd = ax < 3
    if not kd.any():
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros(0, np.float32)
    ax, pos = ax[kd], pos[kd]
    pick = rng.integers(0, ax.shape[0], n)
    a, p = ax[pick], pos[pick]
    rows = np.arange(n)
    o = (blo + rng.uniform(0, 1, (n, 3)) * ext).astype(np.float32)
    o[rows, a] = p
    d = rng.normal(size=(n, 3)).astype(np.float32)
    q = n // 6
    d[rows[:q], a[:q]] = 0.0
    d[rows[q:2 * q], a[q:2 * q]] = -0.0
    d[rows[2 * q:3 * q], a[2 * q:3 * q]] = np.inf
    d[rows[3 * q:4 * q], a[3 * q:4 * q]] = -np.inf
    other = (a + 1) % 3
    o[rows[4 * q:5 * q], other[4 * q:5 * q]] = np.where(rng.uniform(size=q) < 0.5, np.float32(np.inf), np.float32(-np.inf))
    o[rows[5 * q:], other[5 * q:]] = -0.0
    d[rows[5 * q:], a[5 * q:]] = np.where(rng.uniform(size=n - 5 * q) < 0.5, np.float32(0.0), np.float32(-0.0))
    return o, d, np.full(n, np.inf, np.float32)


def test_closest_hit_equals_the_reference_walk(rk):
    _, _, _, sc, tree, ref, oracle, bounds = rk
    for i, (o, d, tm) in enumerate(_rays(tree, ref, oracle, bounds, 20000, 1)):
        if tm.shape[0] == 0:
            continue
        t0, p0, b0, c0 = ref.intersect(o, d, tm)
        t1, p1, b1, c1 = sc.intersect(o, d, tm, count=True)
        assert np.array_equal(p0, p1), (i, int((p0 != p1).sum()))
        assert np.array_equal(_bits(t0), _bits(t1)), i
        assert np.array_equal(_bits(b0), _bits(b1)), i
        assert c1.tolist() == c0[:, :4].sum(0).tolist(), (i, c1, c0.sum(0))
        assert sc.kd_counters() == (int(c0[:, 4].sum()), 0), (i, sc.kd_counters(), c0[:, 4].sum())
        assert c1[1] > 0 and c1[0] > c1[1]


def test_any_hit_equals_the_reference_walk(rk):
    _, _, _, sc, tree, ref, oracle, bounds = rk
    for i, (o, d, tm) in enumerate(_rays(tree, ref, oracle, bounds, 20000, 2)):
        if tm.shape[0] == 0:
            continue
        occ0, c0 = ref.occluded(o, d, tm)
        occ1, c1 = sc.occluded(o, d, tm, count=True)
        assert np.array_equal(occ0, occ1), (i, int((occ0 != occ1).sum()))
        assert c1.tolist() == c0[:, :4].sum(0).tolist(), (i, c1, c0.sum(0))
        assert sc.kd_counters() == (0, int(c0[:, 4].sum())), (i, sc.kd_counters(), c0[:, 4].sum())


def test_separating_rays_tell_the_kd_form_from_the_dot_form(rk):
    """On the separating rays the device follows the kd form; RBSP's dot-product step (the restatement with dot_only, the
    step k_rbspwalk takes) walks some of them differently, so a walk with that step would fail here."""
    _, _, _, sc, tree, ref, _, bounds = rk
    if tree.info()["kd_interior"] == 0:
        pytest.skip("no axis nodes")
    o, d, tm = _separating_rays(tree, bounds, 20000, np.random.default_rng(5))
    t0, p0, b0, c0 = ref.intersect(o, d, tm)
    occ0, q0 = ref.occluded(o, d, tm)
    t1, p1, b1, c1 = sc.intersect(o, d, tm, count=True)
    assert np.array_equal(p0, p1) and np.array_equal(_bits(t0), _bits(t1)) and np.array_equal(_bits(b0), _bits(b1))
    assert c1.tolist() == c0[:, :4].sum(0).tolist()
    occ1, q1 = sc.occluded(o, d, tm, count=True)
    assert np.array_equal(occ0, occ1) and q1.tolist() == q0[:, :4].sum(0).tolist()
    ref.dot_only(True)
    try:
        t2, p2, b2, c2 = ref.intersect(o, d, tm)
        occ2, q2 = ref.occluded(o, d, tm)
    finally:
        ref.dot_only(False)
    differs = (c2 != c0).any(1) | (q2 != q0).any(1) | (p2 != p0) | (_bits(t2) != _bits(t0)) | (occ2 != occ0)
    assert differs.sum() > 0, "no separating ray separates the two forms"


def test_device_entry_points_agree_with_the_host_ones(rk):
    import torch
    _, _, _, sc, tree, ref, oracle, bounds = rk
    o, d, tm = _rays(tree, ref, oracle, bounds, 4096, 3)[1]
    t0, p0, b0 = sc.intersect(o, d, tm)
    occ0 = sc.occluded(o, d, tm)
    n = tm.shape[0]
    rays7 = torch.from_numpy(np.concatenate([o.T, d.T, tm[None]], 0).astype(np.float32).copy()).cuda()
    t = torch.zeros(n, dtype=torch.float32, device="cuda"); p = torch.zeros(n, dtype=torch.int32, device="cuda")
    b = torch.zeros(3 * n, dtype=torch.float32, device="cuda"); occ = torch.zeros(n, dtype=torch.uint8, device="cuda")
    sc.intersect_device(n, rays7.data_ptr(), t.data_ptr(), p.data_ptr(), b.data_ptr())
    sc.occluded_device(n, rays7.data_ptr(), occ.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(p.cpu().numpy(), p0) and np.array_equal(t.cpu().numpy().view(np.uint32), t0.view(np.uint32))
    assert np.array_equal(np.ascontiguousarray(b.cpu().numpy().reshape(3, n).T).view(np.uint32), b0.view(np.uint32))
    assert np.array_equal(occ.cpu().numpy(), occ0)


def test_rbspkd_renders_match_the_reference_images(hprt, rk):
    path, _, m, sc, _, _, _, _ = rk
    opt = m.options.copy()
    opt.spp = 8
    film, st = sc.render(opt)
    rgb = hprt.film_resolve(film, opt.film_scale)
    name = "killeroo_simple" if path == KILLEROO else "dodecahedron"
    ref = np.load(os.path.join(GOLDEN, name + "_8spp_srgb8.npz"))["srgb8"].astype(np.int32)
    d = np.abs(_srgb8(rgb) - ref).astype(np.float64)
    # the tolerances test_gpu_rbsp.py holds the RBSP films to
    if name == "killeroo_simple":
        assert d.mean() < 0.002 and d.max() <= 9 and (d > 2).mean() < 3e-4, (d.mean(), d.max(), (d > 2).mean())
    else:
        assert d.max() == 0, (d.max(), int((d != 0).sum()))


def test_counting_render_pixel_kd_stats(hprt, rk, tmp_path):
    _, M, m, sc, _, _, _, _ = rk
    opt = m.options.copy()
    opt.spp = 2
    for i, c in enumerate((0.4, 0.4 + 48 / 700.0, 0.45, 0.45 + 40 / 700.0)):
        opt.crop[i] = c
    film, st = sc.render(opt, count_work=True, pixel_stats=True)
    kdc = sc.kd_counters()
    px = sc.pixel_stats()
    kd2 = sc.pixel_kd_stats()
    s = px.reshape(-1, 7).sum(0)
    assert s[5] == st["nodes_entered"] and s[6] == st["nodes_entered_p"]
    assert s[3] + s[5] == st["nodes_fetched"] and s[4] + s[6] == st["nodes_fetched_p"]
    assert int(kd2[0].sum()) == kdc[0] and int(kd2[1].sum()) == kdc[1]
    assert (kd2[0] <= px[:, :, 5]).all() and (kd2[1] <= px[:, :, 6]).all()
    assert kdc[0] > 0 and kdc[1] > 0
    if M == 3:
        assert kdc == (st["nodes_entered"], st["nodes_entered_p"])
    hprt.write_pixel_stats_rbspkd(str(tmp_path / "rk"), px, kd2)
    load = lambda n: np.loadtxt(tmp_path / ("rk-%s.txt" % n), dtype=np.uint64).reshape(px.shape[:2])
    assert np.array_equal(load("kdTreeNodeTraversals"), kd2[0]) and np.array_equal(load("kdTreeNodeTraversalsP"), kd2[1])
    assert np.array_equal(load("bspTreeNodeTraversals"), px[:, :, 5] - kd2[0])
    assert np.array_equal(load("bspTreeNodeTraversalsP"), px[:, :, 6] - kd2[1])
    film2, _ = sc.render(opt)
    assert np.array_equal(film.view(np.uint32), film2.view(np.uint32))


def test_tile_sharded_rbspkd_render_merges_bit_identically(hprt, rk):
    _, _, m, sc, _, _, _, _ = rk
    opt = m.options.copy()
    opt.spp = 2
    for i, c in enumerate((0.3, 0.3 + 96 / 700.0, 0.35, 0.35 + 80 / 700.0)):
        opt.crop[i] = c
    full, _ = sc.render(opt)
    parts, recs = [], []
    for r in range(3):
        f, _ = sc.render(opt, tile_begin=r, tile_stride=3, export_foreign=True)
        parts.append(f); recs.append(sc.film_records())
    merged = hprt.film_records_merge(np.sum(parts, 0).astype(np.float32), np.concatenate(recs))
    assert np.array_equal(merged.view(np.uint32), full.view(np.uint32))


def test_attaching_any_tree_replaces_the_others(hprt):
    """kd -> rbsp -> rbspkd -> kd on one scene: each render is the one a scene with only that tree gives, with its counters."""
    m = hprt.Model.load(DODECA)
    opt = m.options.copy(); opt.spp = 2
    trees = {"kd": ("attach_kdtree", hprt.KdTree(m)), "rbsp": ("attach_rbsp", hprt.Rbsp(m, n_directions=7)),
             "rbspkd": ("attach_rbspkd", hprt.RbspKd(m, n_directions=7))}
    alone = {}
    for name, (attach, tree) in trees.items():
        s = hprt.Scene(m, hprt.Bvh(m), device=0)
        getattr(s, attach)(tree)
        alone[name] = s.render(opt, count_work=True) + (s.kd_counters(),)
    assert alone["rbsp"][1]["nodes_entered"] != alone["rbspkd"][1]["nodes_entered"]
    assert alone["rbsp"][2] == (0, 0) and alone["rbspkd"][2][0] > 0
    sc = hprt.Scene(m, hprt.Bvh(m), device=0)
    for name in ("kd", "rbsp", "rbspkd", "kd"):
        attach, tree = trees[name]
        getattr(sc, attach)(tree)
        film, st = sc.render(opt, count_work=True)
        assert np.array_equal(film.view(np.uint32), alone[name][0].view(np.uint32)), name
        assert st["nodes_entered"] == alone[name][1]["nodes_entered"] and st["nodes_fetched"] == alone[name][1]["nodes_fetched"], name
        assert sc.kd_counters() == alone[name][2], name


def test_attach_refusals(hprt):
    m = hprt.Model.load(DODECA)
    sc = hprt.Scene(m, hprt.Bvh(m), device=0)
    rng = np.random.default_rng(0)
    with pytest.raises(hprt.HprtError) as e:
        sc.attach_rbspkd(hprt.RbspKd.from_triangles(rng.uniform(0, 1, (7, 9))))     # not this scene's primitive count
    assert e.value.code == hprt.E_INVALID
    mi = hprt.Model.load(os.path.join(GOLDEN, "simple_instanced.hprt"))
    si = hprt.Scene(mi, hprt.Bvh(mi), device=0)
    with pytest.raises(hprt.HprtError) as e:
        si.attach_rbspkd(hprt.RbspKd.from_triangles(rng.uniform(0, 1, (1, 9))))
    assert e.value.code == hprt.E_UNSUPPORTED
    opt = m.options.copy(); opt.spp = 1
    sc.render(opt)                                       # no rbspkd tree and no pixel statistics: nothing to read
    with pytest.raises(hprt.HprtError) as e:
        sc.pixel_kd_stats()
    assert e.value.code == hprt.E_INVALID


def test_rbspkd_walk_resources(hprt, tmp_path):
    """k_rbspkdwalk's targets are k_rbspwalk's: triangle-only kernels <= 80 registers (six workgroups per CU) with nothing in
    scratch, quadric kernels <= 128 (four); LDS: eight todo entries per lane of a 256-thread workgroup plus the direction table."""
    import yaml
    llvm = "/opt/rocm/lib/llvm/bin"
    lib = os.path.join(ROOT, "thesis-pbrt-v3_amd", "lib", "libhprt.so")
    fat = str(tmp_path / "fat.bin")
    subprocess.run([llvm + "/llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, lib], check=True)
    data = open(fat, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    starts = []
    pos = data.find(magic)
    while pos >= 0:
        starts.append(pos); pos = data.find(magic, pos + 1)
    ks = {}
    for j, s0 in enumerate(starts):
        part, co = str(tmp_path / ("b%d.bin" % j)), str(tmp_path / ("b%d.co" % j))
        open(part, "wb").write(data[s0:starts[j + 1] if j + 1 < len(starts) else len(data)])
        if subprocess.run([llvm + "/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + part, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           "--output=" + co], capture_output=True).returncode != 0 or os.path.getsize(co) == 0:
            continue
        notes = subprocess.run([llvm + "/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
        if "---" not in notes:
            continue
        meta = yaml.safe_load(notes[notes.index("---"):notes.rindex("...")])
        ks.update({k[".name"]: k for k in meta.get("amdhsa.kernels", []) if "k_rbspkdwalk" in k[".name"]})
    assert len(ks) == 8, sorted(ks)
    for name, k in ks.items():
        quad = name.split("k_rbspkdwalkI")[1].split("Lb")[3].startswith("1")      # <ANY_HIT, COUNT, QUAD>
        assert k[".group_segment_fixed_size"] == 8 * 256 * 8 + 4 * 3 * 13, name
        assert k[".vgpr_count"] <= (128 if quad else 80) and k[".vgpr_spill_count"] == 0, (name, k[".vgpr_count"])
        if not quad:
            assert k[".private_segment_fixed_size"] == 0, name
