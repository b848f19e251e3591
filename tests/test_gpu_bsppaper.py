"""The general BSP walk on the GPU (Accelerator "bsppaper"): closest and any hit held bit for bit to the test-side restatement of
BSP::Intersect / IntersectP (tests/bsppaper_reference.cpp) — t, primitive, barycentrics and all four counters — on camera, random,
degenerate, infinite and on-a-split-plane rays; renders against the reference's image; per-pixel statistics; tile sharding;
switching between the BVH, bsppaper, RBSP and kd walks; attach refusals; kernel resources.  Scenes: the dodecahedron and a prefix
of killeroo-simple's triangles with three spheres (the restated build must equal the library's), and killeroo-simple (about 1.5
minutes to build on 16 threads; the restatement walks the library's tree)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import bsppaper_ref

pytestmark = pytest.mark.gpu
DODECA = os.path.join(GOLDEN, "dodecahedron.hprt")
KILLEROO = os.path.join(GOLDEN, "killeroo_simple.hprt")


def _prefix_scene(tmp_path_factory, hprt):
    """killeroo-simple's first 2000 triangles and three spheres (one crossing the mesh), baked"""
    from test_host_side import HEADER
    p9 = bsppaper_ref.BspScene(KILLEROO, build=False).triangles()[:2000]
    P = p9.reshape(-1, 3)
    idx = np.arange(P.shape[0], dtype=np.int32)
    c = P.mean(0); r = float(np.abs(P - c).max())
    spheres = "".join('AttributeBegin Translate %r %r %r Shape "sphere" "float radius" [%r] AttributeEnd\n' % (float(x), float(y), float(z), rad)
                      for (x, y, z), rad in ((c, 0.2 * r), (c + [0.6 * r, 0, 0], 0.1 * r), (c - [0, 0.7 * r, 0.1 * r], 0.15 * r)))
    text = (HEADER + spheres + 'Shape "trianglemesh" "integer indices" [' + " ".join(map(str, idx)) + '] "point P" [' +
            " ".join(repr(float(v)) for v in P.ravel()) + "]\nWorldEnd\n")
    d = tmp_path_factory.mktemp("bsppaper")
    (d / "prefix.pbrt").write_text(text)
    m = hprt.Model.parse(str(d / "prefix.pbrt"))
    m.save(str(d / "prefix.hprt"))
    return str(d / "prefix.hprt")


_SCENES = {}


def _scene(name, hprt, orc, tmp_path_factory):
    """(path, model, scene with the attached bsppaper tree, tree, restatement, oracle or None, BVH bounds), built once per module"""
    if name in _SCENES:
        return _SCENES[name]
    path = {"dodecahedron": DODECA, "killeroo-simple": KILLEROO}.get(name) or _prefix_scene(tmp_path_factory, hprt)
    m = hprt.Model.load(path)
    bvh = hprt.Bvh(m)
    sc = hprt.Scene(m, bvh, device=0)
    tree = hprt.BspPaper(m)
    sc.attach_bsppaper(tree)
    nodes, idx = tree.arrays()
    if name != "killeroo-simple":
        ref = bsppaper_ref.BspScene(path)                 # the restated build: the library's tree must be the same
        rn, ri = ref.tree()
        interior = (nodes[:, 1] & 1) == 0
        assert np.array_equal(nodes[:, :2], rn[:, :2]) and np.array_equal(nodes[interior], rn[interior]) and np.array_equal(idx, ri)
    else:
        ref = bsppaper_ref.BspScene(path, build=False)    # killeroo-simple's restated build is slow: walk the library's tree
        ref.set_tree(nodes, idx)
    b = np.array(bvh.info()["bounds"], np.float32)
    _SCENES[name] = (path, m, sc, tree, ref, orc.OracleScene(path) if name != "killeroo-prefix-spheres" else None, (b[:3], b[3:]))
    return _SCENES[name]


@pytest.fixture(scope="module", params=["dodecahedron", "killeroo-simple", "killeroo-prefix-spheres"])
def walked(request, hprt, orc, tmp_path_factory):
    """the scenes the walks are held to the restatement on"""
    return _scene(request.param, hprt, orc, tmp_path_factory)


@pytest.fixture(scope="module", params=["dodecahedron", "killeroo-simple"])
def bp(request, hprt, orc, tmp_path_factory):
    """the scenes with the reference's camera and image"""
    return _scene(request.param, hprt, orc, tmp_path_factory)


@pytest.fixture(scope="module")
def quad(hprt, orc, tmp_path_factory):
    return _scene("killeroo-prefix-spheres", hprt, orc, tmp_path_factory)


def _dot32(d, o):
    """Dot(axis, o) in float32, x*x + y*y + z*z left to right (one rounding per operation)"""
    d = d.astype(np.float32); o = o.astype(np.float32)
    return ((d[..., 0] * o[..., 0] + d[..., 1] * o[..., 1]) + d[..., 2] * o[..., 2]).astype(np.float32)


def _on_plane(axes, pos, o):
    """Move each origin onto its split plane so that the float Dot(axis, o) equals the split exactly: project, then step the
    coordinate with the largest axis component by nextafter.  Returns the origins and which of them made it."""
    d = axes.astype(np.float64)
    o = (o + (pos.astype(np.float64) - (o.astype(np.float64) * d).sum(1))[:, None] * d).astype(np.float32)
    k = np.abs(axes).argmax(1)
    rows = np.arange(o.shape[0])
    for _ in range(200):
        v = _dot32(axes, o)
        bad = v != pos
        if not bad.any():
            break
        up = (v < pos) == (axes[rows, k] > 0)
        cur = o[rows, k]
        o[rows, k] = np.where(bad, np.nextafter(cur, np.where(up, np.float32(np.inf), np.float32(-np.inf))).astype(np.float32), cur)
    return o, _dot32(axes, o) == pos


def _rays(tree, oracle, bounds, n, seed):
    rng = np.random.default_rng(seed)
    blo, bhi = bounds
    ext = bhi - blo
    out = []
    if oracle is not None:      # camera rays
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
    # origins whose float Dot(axis, o) equals a node's split exactly (the belowFirst tie), triangle planes included; a third of
    # them with Dot(axis, d) == 0 (the direction's components zeroed along the axis's support, or d made perpendicular to it)
    nodes, _ = tree.arrays()
    inner = np.nonzero((nodes[:, 1] & 1) == 0)[0]
    pick = inner[rng.integers(0, inner.shape[0], n)]
    axes = nodes[pick, 2:].view(np.float32).copy()
    pos = nodes[pick, 0].view(np.float32).copy()
    o = (blo + rng.uniform(0, 1, (n, 3)) * ext).astype(np.float32)
    o, ok = _on_plane(axes, pos, o)
    assert ok.mean() > 0.5, ok.mean()
    d = rng.normal(size=(n, 3)).astype(np.float32)
    third = n // 3
    d[:third] = np.where(axes[:third] != 0, np.float32(0.0), d[:third])
    d[third:2 * third, rng.integers(0, 3)] = -0.0
    out.append((o[ok], d[ok], np.full(int(ok.sum()), np.inf, np.float32)))
    return out


def _bits(a):
    a = np.where(np.isnan(a), np.float32(np.nan), a).astype(np.float32)
    return a.view(np.uint32)


def test_closest_hit_equals_the_reference_walk(walked):
    _, _, sc, tree, ref, oracle, bounds = walked
    for i, (o, d, tm) in enumerate(_rays(tree, oracle, bounds, 20000, 1)):
        t0, p0, b0, c0 = ref.intersect(o, d, tm)
        t1, p1, b1, c1 = sc.intersect(o, d, tm, count=True)
        assert np.array_equal(p0, p1), (i, int((p0 != p1).sum()))
        assert np.array_equal(_bits(t0), _bits(t1)), i
        assert np.array_equal(_bits(b0), _bits(b1)), i
        assert c1.tolist() == c0.sum(0).tolist(), (i, c1, c0.sum(0))
        assert c1[1] > 0 and c1[0] > c1[1]


def test_any_hit_equals_the_reference_walk(walked):
    _, _, sc, tree, ref, oracle, bounds = walked
    for i, (o, d, tm) in enumerate(_rays(tree, oracle, bounds, 20000, 2)):
        occ0, c0 = ref.occluded(o, d, tm)
        occ1, c1 = sc.occluded(o, d, tm, count=True)
        assert np.array_equal(occ0, occ1), (i, int((occ0 != occ1).sum()))
        assert c1.tolist() == c0.sum(0).tolist(), (i, c1, c0.sum(0))


def test_quadric_variants_ran(quad):
    path, m, sc, tree, ref, oracle, bounds = quad
    o, d, tm = _rays(tree, oracle, bounds, 4096, 5)[0]
    _, _, _, c = sc.intersect(o, d, tm, count=True)
    assert c[3] > 0      # sphere tests: the QUAD kernels walked


def _srgb8(rgb):
    v = rgb.astype(np.float64)
    g = np.where(v <= 0.0031308, 12.92 * v, 1.055 * np.power(np.maximum(v, 1e-30), 1 / 2.4) - 0.055)
    return np.clip(255.0 * g + 0.5, 0, 255).astype(np.int32)


def test_bsppaper_renders_match_the_reference_images(hprt, bp):
    path, m, sc, _, _, _, _ = bp
    opt = m.options.copy()
    opt.spp = 8
    film, _ = sc.render(opt)
    rgb = hprt.film_resolve(film, opt.film_scale)
    name = "killeroo_simple" if path == KILLEROO else "dodecahedron"
    ref = np.load(os.path.join(GOLDEN, name + "_8spp_srgb8.npz"))["srgb8"].astype(np.int32)
    d = np.abs(_srgb8(rgb) - ref).astype(np.float64)
    # the tolerances the BVH, kd and rbsp films are held to (tests/test_gpu_rbsp.py)
    if name == "killeroo_simple":
        assert d.mean() < 0.002 and d.max() <= 9 and (d > 2).mean() < 3e-4, (d.mean(), d.max(), (d > 2).mean())
    else:
        assert d.max() == 0, (d.max(), int((d != 0).sum()))


def test_counting_render_pixel_stats(hprt, bp, tmp_path):
    path, m, sc, _, _, _, _ = bp
    opt = m.options.copy()
    opt.spp = 2
    for i, c in enumerate((0.4, 0.4 + 48 / 700.0, 0.45, 0.45 + 40 / 700.0)):
        opt.crop[i] = c
    film, st = sc.render(opt, count_work=True, pixel_stats=True)
    px = sc.pixel_stats()
    s = px.reshape(-1, 7).sum(0)
    assert s[5] > 0 and s[6] > 0 and s[3] > 0
    assert s[5] == st["nodes_entered"] and s[6] == st["nodes_entered_p"]
    assert s[3] + s[5] == st["nodes_fetched"] and s[4] + s[6] == st["nodes_fetched_p"]
    hprt.write_pixel_stats_accel(str(tmp_path / "bp"), px, hprt.ACCEL_BSP)
    assert np.array_equal(np.loadtxt(tmp_path / "bp-bspTreeNodeTraversals.txt", dtype=np.uint64).reshape(px.shape[:2]), px[:, :, 5])
    film2, _ = sc.render(opt)
    assert np.array_equal(film.view(np.uint32), film2.view(np.uint32))


def test_tile_sharded_render_merges_bit_identically(hprt, bp):
    path, m, sc, _, _, _, _ = bp
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


def test_switching_walks_and_failed_attach(hprt):
    """BVH, then bsppaper, then rbsp, then kd: each render is the one a scene with only that walk gives; a refused attach leaves
    the walk before it in place."""
    m = hprt.Model.load(DODECA)
    opt = m.options.copy(); opt.spp = 2
    trees = {"bsppaper": ("attach_bsppaper", hprt.BspPaper(m)), "rbsp": ("attach_rbsp", hprt.Rbsp(m, n_directions=7)), "kd": ("attach_kdtree", hprt.KdTree(m))}
    alone = {"bvh": hprt.Scene(m, hprt.Bvh(m), device=0).render(opt, count_work=True)}
    for name, (attach, tree) in trees.items():
        s = hprt.Scene(m, hprt.Bvh(m), device=0)
        getattr(s, attach)(tree)
        alone[name] = s.render(opt, count_work=True)
    assert alone["bsppaper"][1]["nodes_entered"] != alone["rbsp"][1]["nodes_entered"]
    sc = hprt.Scene(m, hprt.Bvh(m), device=0)
    bad = hprt.BspPaper.from_triangles(np.random.default_rng(0).uniform(0, 1, (7, 9)))      # not this scene's primitive count
    for name in ("bvh", "bsppaper", "rbsp", "kd"):
        if name != "bvh":
            getattr(sc, trees[name][0])(trees[name][1])
        film, st = sc.render(opt, count_work=True)
        assert np.array_equal(film.view(np.uint32), alone[name][0].view(np.uint32)), name
        assert st["nodes_entered"] == alone[name][1]["nodes_entered"] and st["nodes_fetched"] == alone[name][1]["nodes_fetched"], name
        with pytest.raises(hprt.HprtError) as e:
            sc.attach_bsppaper(bad)
        assert e.value.code == hprt.E_INVALID
        film, st = sc.render(opt, count_work=True)
        assert np.array_equal(film.view(np.uint32), alone[name][0].view(np.uint32)), name + " after a refused attach"


def test_attach_refusals(hprt):
    mi = hprt.Model.load(os.path.join(GOLDEN, "simple_instanced.hprt"))
    si = hprt.Scene(mi, hprt.Bvh(mi), device=0)
    with pytest.raises(hprt.HprtError) as e:
        si.attach_bsppaper(hprt.BspPaper.from_triangles(np.random.default_rng(0).uniform(0, 1, (1, 9))))
    assert e.value.code == hprt.E_UNSUPPORTED
    with pytest.raises(hprt.HprtError) as e:
        hprt.BspPaper(mi)
    assert e.value.code == hprt.E_UNSUPPORTED


def test_bsppaper_walk_resources(hprt, tmp_path):
    """Triangle-only kernels: <= 80 registers (six workgroups per CU), nothing in scratch; quadric kernels <= 128 (four, as the
    RBSP walk's); LDS: eight 8-byte todo entries per lane of a 256-thread workgroup."""
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
        ks.update({k[".name"]: k for k in meta.get("amdhsa.kernels", []) if "k_bsppaperwalk" in k[".name"]})
    assert len(ks) == 8, sorted(ks)
    for name, k in ks.items():
        quad = name.split("k_bsppaperwalkI")[1].split("Lb")[3].startswith("1")      # <ANY_HIT, COUNT, QUAD>
        assert k[".group_segment_fixed_size"] == 8 * 256 * 8, name
        assert k[".vgpr_count"] <= (128 if quad else 80) and k[".vgpr_spill_count"] == 0, (name, k[".vgpr_count"])
        if not quad:
            assert k[".private_segment_fixed_size"] == 0, name
