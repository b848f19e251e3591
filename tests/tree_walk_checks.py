"""What the GPU parity tests of the tree accelerators share (tests/test_gpu_{kdtree,rbsp,rbspkd,bsppaper}.py): the bit views,
the ray families that are generated alike, the checks of a device walk against its test-side restatement, of a render against
the reference's image, of the counting render and of tile sharding, and the reader of the kernel metadata in libhprt.so.
The generators take the caller's np.random.default_rng and draw from it in a fixed order: a file's _rays strings them together
with its own families, and a change of that order changes every later ray."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
KILLEROO = os.path.join(GOLDEN, "killeroo_simple.hprt")
LLVM = "/opt/rocm/lib/llvm/bin"
LIBHPRT = os.path.join(ROOT, "thesis-pbrt-v3_amd", "lib", "libhprt.so")


def _bits(a):
    """float bits with every NaN made one: a NaN direction gives a NaN "hit" in both walks (every comparison of the triangle
    test is false), but the host's and the device's NaNs carry different sign / payload bits"""
    a = np.where(np.isnan(a), np.float32(np.nan), a).astype(np.float32)
    return a.view(np.uint32)


def _srgb8(rgb):
    v = rgb.astype(np.float64)
    g = np.where(v <= 0.0031308, 12.92 * v, 1.055 * np.power(np.maximum(v, 1e-30), 1 / 2.4) - 0.055)
    return np.clip(255.0 * g + 0.5, 0, 255).astype(np.int32)


def _dot32(d, o):
    """Dot(direction, o) in float32, x*x + y*y + z*z left to right (one rounding per operation)"""
    d = d.astype(np.float32); o = o.astype(np.float32)
    return ((d[..., 0] * o[..., 0] + d[..., 1] * o[..., 1]) + d[..., 2] * o[..., 2]).astype(np.float32)


def _on_plane(axes, pos, o):
    """Move each origin onto its split plane (axes[i], pos[i]) so that the float Dot(axis, o) equals the split exactly: project,
    then step the coordinate with the largest axis component by nextafter.  Returns the origins and which of them made it."""
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


def camera_rays(rng, oracle, n):
    o, d = oracle.camera_rays(rng.integers(0, 700, n).astype(np.int32), rng.integers(0, 700, n).astype(np.int32), rng.integers(0, 8, n).astype(np.int64))
    return o, d, np.full(n, np.inf, np.float32)


def random_rays(rng, blo, ext, n):
    """random rays from inside and around the scene, finite and infinite"""
    o = (blo + rng.uniform(-0.2, 1.2, (n, 3)) * ext).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    tm = np.where(rng.uniform(size=n) < 0.5, np.inf, rng.uniform(0, 1, n) * np.linalg.norm(ext)).astype(np.float32)
    return o, d, tm


def degenerate_rays(rng, blo, ext, n):
    """zero direction components of either sign next to non-zero ones, -0 origins, NaN / +-inf directions and origins"""
    o = (blo + rng.uniform(-0.2, 1.2, (n, 3)) * ext).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    k = n // 10
    d[:k, 0] = 0.0; d[k:2 * k, 1] = -0.0; d[2 * k:3 * k, 0] = -0.0; d[2 * k:3 * k, 2] = 0.0
    d[3 * k:4 * k, 0] = -0.0; d[3 * k:4 * k, 1:] = np.abs(d[3 * k:4 * k, 1:])     # 1 / Dot(x, d) = +inf where kd's invDir.x is -inf
    o[3 * k:4 * k, 0] = -0.0
    d[4 * k:4 * k + 8] = np.nan; d[4 * k + 8:4 * k + 16, 1] = np.inf; d[4 * k + 16:4 * k + 24, 2] = -np.inf
    o[4 * k + 24:4 * k + 32, 0] = np.inf
    return o, d, np.full(n, np.inf, np.float32)


def plane_tie_rays(rng, blo, ext, n, axes, pos):
    """Origins whose float Dot(axis, o) equals a split exactly (the belowFirst tie), on planes drawn from the caller's (axes
    [P, 3], pos [P]); a third of them with the direction's components zeroed along the axis's support (Dot(axis, d) == 0), a
    third with one -0 component."""
    pick = rng.integers(0, pos.shape[0], n)
    axes, pos = axes[pick], pos[pick]
    o = (blo + rng.uniform(0, 1, (n, 3)) * ext).astype(np.float32)
    o, ok = _on_plane(axes, pos, o)
    assert ok.mean() > 0.5, ok.mean()
    d = rng.normal(size=(n, 3)).astype(np.float32)
    third = n // 3
    d[:third] = np.where(axes[:third] != 0, np.float32(0.0), d[:third])
    d[third:2 * third, rng.integers(0, 3)] = -0.0
    return o[ok], d[ok], np.full(int(ok.sum()), np.inf, np.float32)


def check_closest(sc, ref, rays):
    """the device's closest hits on each ray family are the restatement's: primitive, t, barycentrics and the summed counters
    (with a fifth counter column, the kd share too)"""
    for i, (o, d, tm) in enumerate(rays):
        t0, p0, b0, c0 = ref.intersect(o, d, tm)
        t1, p1, b1, c1 = sc.intersect(o, d, tm, count=True)
        assert np.array_equal(p0, p1), (i, int((p0 != p1).sum()))
        assert np.array_equal(_bits(t0), _bits(t1)), i
        assert np.array_equal(_bits(b0), _bits(b1)), i
        assert c1.tolist() == c0[:, :4].sum(0).tolist(), (i, c1, c0.sum(0))
        if c0.shape[1] == 5:
            assert sc.kd_counters() == (int(c0[:, 4].sum()), 0), (i, sc.kd_counters(), c0[:, 4].sum())
        assert c1[1] > 0 and c1[0] > c1[1]


def check_any(sc, ref, rays):
    for i, (o, d, tm) in enumerate(rays):
        occ0, c0 = ref.occluded(o, d, tm)
        occ1, c1 = sc.occluded(o, d, tm, count=True)
        assert np.array_equal(occ0, occ1), (i, int((occ0 != occ1).sum()))
        assert c1.tolist() == c0[:, :4].sum(0).tolist(), (i, c1, c0.sum(0))
        if c0.shape[1] == 5:
            assert sc.kd_counters() == (0, int(c0[:, 4].sum())), (i, sc.kd_counters(), c0[:, 4].sum())


def check_device_entry_points(sc, o, d, tm):
    """hprt_intersect_device / hprt_occluded_device on device buffers give what the host entry points give"""
    import torch
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


def check_reference_image(hprt, sc, m, path):
    """an 8 spp render against the reference's image, to the tolerances the BVH films are held to (tests/test_oracle_pins.py)"""
    opt = m.options.copy()
    opt.spp = 8
    film, _ = sc.render(opt)
    rgb = hprt.film_resolve(film, opt.film_scale)
    name = "killeroo_simple" if path == KILLEROO else "dodecahedron"
    ref = np.load(os.path.join(GOLDEN, name + "_8spp_srgb8.npz"))["srgb8"].astype(np.int32)
    d = np.abs(_srgb8(rgb) - ref).astype(np.float64)
    if name == "killeroo_simple":
        assert d.mean() < 0.002 and d.max() <= 9 and (d > 2).mean() < 3e-4, (d.mean(), d.max(), (d > 2).mean())
    else:
        assert d.max() == 0, (d.max(), int((d != 0).sum()))


def check_counting_render(sc, m):
    """A counting render of a small crop with per-pixel statistics: the pixels' sums are the render's counters.  Returns the
    render's counters and the per-pixel array for the caller's own checks, and a function that checks, last of all (a plain
    render clears the scene's statistics), that the counted render's film is the plain render's."""
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
    assert s[1] == st["tri_tests"] + st["sphere_tests"] and s[2] == st["tri_tests_p"] + st["sphere_tests_p"]

    def check_plain_film():
        film2, _ = sc.render(opt)
        assert np.array_equal(film.view(np.uint32), film2.view(np.uint32))
    return st, px, check_plain_film


def check_tile_sharding(hprt, sc, m):
    """three tile-strided renders with exported foreign records merge into the full render bit for bit"""
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


def kernel_metadata(lib, tmp):
    """{kernel name: its amdhsa metadata} of every gfx950 code object in `lib` (one offload bundle per translation unit)"""
    import yaml
    fat = os.path.join(str(tmp), "fat.bin")
    subprocess.run([LLVM + "/llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, lib], check=True)
    data = open(fat, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    starts = []
    pos = data.find(magic)
    while pos >= 0:
        starts.append(pos); pos = data.find(magic, pos + 1)
    ks = {}
    for j, s0 in enumerate(starts):
        part, co = os.path.join(str(tmp), "b%d.bin" % j), os.path.join(str(tmp), "b%d.co" % j)
        open(part, "wb").write(data[s0:starts[j + 1] if j + 1 < len(starts) else len(data)])
        if subprocess.run([LLVM + "/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + part, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           "--output=" + co], capture_output=True).returncode != 0 or os.path.getsize(co) == 0:
            continue
        notes = subprocess.run([LLVM + "/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
        if "---" not in notes:
            continue
        meta = yaml.safe_load(notes[notes.index("---"):notes.rindex("...")])
        ks.update({k[".name"]: k for k in meta.get("amdhsa.kernels", [])})
    return ks


def check_walk_resources(tmp, kernel, lds):
    """The eight variants <ANY_HIT, COUNT, QUAD> of a walk kernel: triangle-only ones <= 80 registers (six workgroups per CU) with
    nothing in scratch, quadric ones <= 128 (four); none spills; `lds` bytes of LDS."""
    ks = {n: k for n, k in kernel_metadata(LIBHPRT, tmp).items() if kernel in n}
    assert len(ks) == 8, sorted(ks)
    for name, k in ks.items():
        quad = name.split(kernel + "I")[1].split("Lb")[3].startswith("1")
        assert k[".group_segment_fixed_size"] == lds, name
        assert k[".vgpr_count"] <= (128 if quad else 80) and k[".vgpr_spill_count"] == 0, (name, k[".vgpr_count"])
        if not quad:
            assert k[".private_segment_fixed_size"] == 0, name
