"""Shadow rays of a render replayed through the any-hit walk and through the light-centred grid.

Renders <spp> samples of a bench workload, captures the shadow rays that bounces 1 and 2 queue (hprt_debug_capture_rays), and
replays each set, in the order the render queued it, through hprt_occluded_device (k_walk4<any hit>) and through k_shadow_grid
(hprt_debug_shadow_grid_occluded) at several grid resolutions, a few times each in one session; the answers must agree.  At
64 spp the atrium's sets hold ~25 M rays (~800 MB): several times the Infinity Cache, which a small set would sit in.
Usage: shadow_grid_replay.py [workload] [spp] [R ...]      (default: atrium 64 256 512 1024)"""
import importlib, os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
hprt = importlib.import_module("thesis-pbrt-v3_amd")
name = sys.argv[1] if len(sys.argv) > 1 else "atrium"
spp = int(sys.argv[2]) if len(sys.argv) > 2 else 64
res = [int(x) for x in sys.argv[3:]] or [256, 512, 1024]
ITERS = 4
dev = torch.device("cuda", 0)
model = bench.build_model(hprt, name); bvh = hprt.Bvh(model)


def make_scene(R):
    os.environ["HPRT_SHADOW_GRID_RES"] = str(R); os.environ["HPRT_SHADOW_GRID"] = "1"      # (a grid whatever its lists' lengths)
    try:
        return hprt.Scene(model, bvh, device=0)
    finally:
        del os.environ["HPRT_SHADOW_GRID_RES"], os.environ["HPRT_SHADOW_GRID"]


scenes = {R: make_scene(R) for R in res}
for R, s in scenes.items():
    print("grid R=%d: %s" % (R, s.shadow_grid_info()), flush=True)
scene = scenes[res[0]]
opt = model.options.copy(); opt.spp = spp
x0, y0, x1, y1 = opt.film_bounds()
cap = (x1 - x0) * (y1 - y0) * spp
import ctypes as C
lib = hprt.lib
lib.hprt_debug_capture_rays.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
lib.hprt_debug_captured.restype = C.c_longlong; lib.hprt_debug_captured.argtypes = [C.c_void_p]
lib.hprt_debug_trace_queued.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_float)]


def capture(bounce):
    buf = torch.zeros(7 * cap, dtype=torch.float32, device=dev)
    hprt._check(lib.hprt_debug_capture_rays(scene._h, bounce, 1, buf.data_ptr(), cap))
    scene.render(opt, spp_chunk=spp)
    n = int(lib.hprt_debug_captured(scene._h))
    hprt._check(lib.hprt_debug_capture_rays(scene._h, -1, 0, None, 0))
    rays = buf.view(7, cap)[:, :n].contiguous()
    del buf
    return rays, n


def timed(fn):
    fn(); torch.cuda.synchronize()
    ms = []
    for _ in range(ITERS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


for bounce in (1, 2):
    rays, n = capture(bounce)
    if n == 0:
        continue
    print("== %s, %d spp: %d shadow rays of bounce %d (%.0f MB)" % (name, spp, n, bounce, 28e-6 * n), flush=True)
    occ_walk = torch.empty(n, dtype=torch.uint8, device=dev)
    scene.occluded_device(n, rays.data_ptr(), occ_walk.data_ptr()); torch.cuda.synchronize()
    # the walk alone (without the packing of the rays into streams): hprt_debug_trace_queued through the identity queue
    queue = torch.arange(n, dtype=torch.int32, device=dev); scratch = torch.empty(7 * n, dtype=torch.float32, device=dev)
    ms2 = (C.c_float * 2)(); ms = []
    for _ in range(ITERS + 1):
        hprt._check(lib.hprt_debug_trace_queued(scene._h, n, rays.data_ptr(), queue.data_ptr(), 1, scratch.data_ptr(), ms2))
        ms.append(ms2[1])
    ms = ms[1:]
    del queue, scratch
    print("  k_walk4<any>           %s ms   best %.1f Mrays/s" % (" ".join("%7.2f" % m for m in ms), n / min(ms) / 1e3), flush=True)
    for R, s in scenes.items():
        occ = torch.empty(n, dtype=torch.uint8, device=dev)
        kernel = []
        ms = timed(lambda: kernel.append(s.shadow_grid_occluded_device(n, rays.data_ptr(), occ.data_ptr())))
        same = bool(torch.equal(occ, occ_walk))
        ms = kernel[1:]      # (the kernel alone, as the walk's figure)
        print("  k_shadow_grid R=%-5d   %s ms   best %.1f Mrays/s   answers identical: %s, occluded %.1f %%"
              % (R, " ".join("%7.2f" % m for m in ms), n / min(ms) / 1e3, same, 100.0 * float(occ.float().mean())), flush=True)
        del occ
    del rays, occ_walk
