"""What a render's shadow rays read of the light-centred grid, counted on the host: entries read, rectangle failures,
candidates tested and distinct 128-byte lines per ray, for the CSR layout k_shadow_grid read before (cellStart pair, 8-byte entries
in pairs, 48-byte triangle records gathered from the ordered triangle array) and for the device image it reads now (a 128-byte block
per cell with two candidates in place, 48-byte records for the rest; csrc/shadow_grid.h).

Renders <spp> samples of a bench workload, captures the shadow rays that bounces 1 and 2 queue (hprt_debug_capture_rays, as
tools/shadow_grid_replay.py), keeps a random <sample> of each set, reads the scene's image back (hprt_debug_shadow_grid_image_read)
and follows every sampled ray through its cell's list as the kernel does — the kernel's cell function restated in float32
(tests/shadow_grid_cases.py), its key cut and rectangle filter — with a double-precision triangle test deciding where a ray stops
(the leaf-box test after a reported hit is left out: it lets a ray go on that this count stops).  Only the capture needs the GPU.
Usage: shadow_grid_lines.py [workload] [spp] [sample]      (default: atrium 64 400000)"""
import importlib, os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench
import shadow_grid_cases as sgc
hprt = importlib.import_module("thesis-pbrt-v3_amd")


def tables(im, near):
    """the image's lists as flat arrays, and the record of every entry (-1: it stands in a block slot)"""
    global cs, count, prim, keyw, key, verts, records_at, rec
    cs, count = im["cell_start"], im["count"]
    prim = (im["prim_word"] & np.uint32(hprt.SG_PRIM_MASK)).astype(np.int64)
    keyw = im["key_word"]
    key = (keyw & np.uint32(0xffff0000)).view(np.float32)
    verts = im["verts"].view(np.float32)
    records_at = im["blocks"].size * 4
    # the record of every entry of the image (-1: it stands in a block slot)
    over = np.maximum(count - hprt.SG_BLOCK_SLOTS, 0)
    slot = np.arange(cs[0], cs[-1]) - np.repeat(cs[:-1], count)
    rec = np.full(int(cs[-1]), -1, np.int64)
    rec[:near] = np.arange(near)
    rec[near:] = np.where(slot >= hprt.SG_BLOCK_SLOTS, np.repeat(im["overflow"], count) + slot - hprt.SG_BLOCK_SLOTS, -1)


def hits(o, d, tmax, v):
    """Moeller-Trumbore in double: the segment o + t d, 0 < t < tmax, meets the triangle v [n, 9]"""
    o, d = o.astype(np.float64), d.astype(np.float64)
    p0, p1, p2 = v[:, 0:3].astype(np.float64), v[:, 3:6].astype(np.float64), v[:, 6:9].astype(np.float64)
    e1, e2 = p1 - p0, p2 - p0
    pv = np.cross(d, e2)
    det = (e1 * pv).sum(1)
    with np.errstate(all="ignore"):
        inv = 1.0 / det
        tv = o - p0
        u = (tv * pv).sum(1) * inv
        qv = np.cross(tv, e1)
        w = (d * qv).sum(1) * inv
        t = (e2 * qv).sum(1) * inv
        return (det != 0) & (u >= 0) & (w >= 0) & (u + w <= 1) & (t > 0) & (t < tmax)


def lines_of(space, lo, hi):
    """the 128-byte lines of bytes [lo, hi) of an array, tagged with the array"""
    a, b = lo // 128, (hi - 1) // 128
    return [space * (1 << 40) + a, space * (1 << 40) + b]


def count_rays(rays, R, near):
    o, d, tmax = rays[0:3].T.copy(), rays[3:6].T.copy(), rays[6].astype(np.float64)
    n = o.shape[0]
    d32 = d.astype(np.float32)
    dist2 = (d32[:, 0] * d32[:, 0] + d32[:, 1] * d32[:, 1]).astype(np.float32) + d32[:, 2] * d32[:, 2]
    lim = np.where(rays[6] <= 1, (dist2 * np.float32(1 + 2.0 ** -20)).astype(np.float32), np.float32(np.inf))
    cell, su, sv = sgc.cell_of(d32, R)
    read = np.zeros(n, np.int64); rect_fail = np.zeros(n, np.int64); tested = np.zeros(n, np.int64); occluded = np.zeros(n, bool)
    csr, img = [], []      # (ray, line) pairs of the two layouts
    ray = np.arange(n)
    for r, l in zip([ray, ray], lines_of(1, cell * 4, cell * 4 + 8)):
        csr.append((r, l))
    img.append((ray, 4 * (1 << 40) + cell))      # the block: one line
    alive = np.ones(n, bool)
    for first, length, is_near in ((np.zeros(n, np.int64), np.full(n, near), True), (cs[cell], count[cell], False)):
        k = 0
        while True:
            act = np.nonzero(alive & (length > k))[0]
            if act.size == 0:
                break
            e = first[act] + k
            read[act] += 1
            # the CSR kernel reads entries in pairs: entry e, and with it e + 1 where the list has one
            for l in lines_of(2, e * 8, e * 8 + np.where(length[act] > k + 1, 16, 8)):
                csr.append((act, l))
            inside = key[e] <= lim[act]
            if not is_near:
                alive[act[~inside]] = False      # the key cut ends the cell's list
            act, e = act[inside], e[inside]
            if is_near or k >= hprt.SG_BLOCK_SLOTS:
                # the image kernel knows the key word of entry k >= 2 beforehand and fetches its record only inside the cut
                for l in lines_of(4, records_at + rec[e] * 48, records_at + rec[e] * 48 + 48):
                    img.append((act, l))
            w = keyw[e]
            reach = (su[act] >= (w & 15)) & (su[act] <= ((w >> 4) & 15)) & (sv[act] >= ((w >> 8) & 15)) & (sv[act] <= ((w >> 12) & 15))
            rect_fail[act[~reach]] += 1
            act, e = act[reach], e[reach]
            tested[act] += 1
            for l in lines_of(3, prim[e] * 48, prim[e] * 48 + 48):
                csr.append((act, l))
            h = hits(o[act], d[act], tmax[act], verts[e])
            occluded[act[h]] = True
            alive[act[h]] = False
            k += 1
        alive = ~occluded

    def distinct(pairs):
        u = np.unique(np.concatenate([(np.asarray(a, np.int64) << 43) | np.asarray(b, np.int64) for a, b in pairs]))
        return np.bincount(u >> 43, minlength=n)

    return read, rect_fail, tested, occluded, distinct(csr), distinct(img)


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "atrium"
    spp = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    sample = int(sys.argv[3]) if len(sys.argv) > 3 else 400000
    dev = torch.device("cuda", 0)
    model = bench.build_model(hprt, name); scene = hprt.Scene(model, hprt.Bvh(model), device=0)
    info = scene.shadow_grid_info()
    print("grid: %s" % info, flush=True)
    assert info["eligible"], "the workload's scene has no shadow grid"
    R, near = info["R"], info["near"]
    opt = model.options.copy(); opt.spp = spp
    x0, y0, x1, y1 = opt.film_bounds()
    cap = (x1 - x0) * (y1 - y0) * spp
    import ctypes as C
    lib = hprt.lib
    lib.hprt_debug_capture_rays.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    lib.hprt_debug_captured.restype = C.c_longlong; lib.hprt_debug_captured.argtypes = [C.c_void_p]
    def capture(bounce):
        buf = torch.zeros(7 * cap, dtype=torch.float32, device=dev)
        hprt._check(lib.hprt_debug_capture_rays(scene._h, bounce, 1, buf.data_ptr(), cap))
        scene.render(opt, spp_chunk=spp)
        n = int(lib.hprt_debug_captured(scene._h))
        hprt._check(lib.hprt_debug_capture_rays(scene._h, -1, 0, None, 0))
        pick = torch.randperm(n, device=dev, generator=torch.Generator(device=dev).manual_seed(bounce))[:sample]
        rays = buf.view(7, cap)[:, pick].cpu().numpy()
        del buf
        return rays, n

    sets = {b: capture(b) for b in (1, 2)}
    tables(scene.shadow_grid_image(), near)
    for bounce, (rays, total) in sets.items():
        if rays.shape[1] == 0:
            continue
        read, rect_fail, tested, occluded, csr, img = count_rays(rays, R, near)
        visited = np.minimum(read, 5)
        print("== %s, %d spp, bounce %d: %d of %d shadow rays, R = %d" % (name, spp, bounce, rays.shape[1], total, R))
        print("   entries read %.2f   rectangle failures %.2f   candidates tested %.2f   occluded %.1f %%"
              % (read.mean(), rect_fail.mean(), tested.mean(), 100.0 * occluded.mean()))
        print("   entries read, histogram 0 1 2 3 4 5+: %s" % " ".join("%.3f" % f for f in np.bincount(visited, minlength=6) / visited.size))
        print("   answer known from the block alone (no record read): %.1f %%" % (100.0 * (img == 1).mean()))
        print("   distinct 128-byte lines per ray, list side: CSR layout %.2f   device image %.2f" % (csr.mean(), img.mean()), flush=True)


if __name__ == "__main__":
    main()
