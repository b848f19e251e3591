"""Shadow rays of a distant-lit render replayed through the any-hit walk and through the light-aligned grid.

The sibling of shadow_grid_replay.py: renders <spp> samples of a scene lit by one distant light, captures the shadow rays that bounces
0 (the camera rays' hits), 1 and 2 queue (hprt_debug_capture_rays), and replays each set, in the order the render queued it, through the walk (k_walk4<any hit>,
hprt_debug_trace_queued) and through k_distant_grid (hprt_debug_distant_grid_occluded) at several grid resolutions, a few times each
in one session; every answer must agree.
Scenes: killeroo — tests/golden/killeroo.hprt as it is (700 x 700, the thesis' scene); atrium — tools/scene_gen.py's atrium with its
light line replaced by a distant light from above at a slant (the hall is closed: every ray from inside ends at the ceiling);
atrium-open — the same without the ceiling mesh.
Usage: distant_grid_replay.py [scene] [spp] [R ...]      (default: killeroo 16 512 1024 2048)"""
import ctypes as C
import importlib, os, re, sys, tempfile
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import scene_gen
hprt = importlib.import_module("thesis-pbrt-v3_amd")
name = sys.argv[1] if len(sys.argv) > 1 else "killeroo"
spp = int(sys.argv[2]) if len(sys.argv) > 2 else 16
res = [int(x) for x in sys.argv[3:]] or [512, 1024, 2048]
ITERS = 4
DISTANT = 'LightSource "distant" "point from" [0.3 -0.2 1] "point to" [0 0 0] "color L" [3.2 3.1 2.9]\n'
dev = torch.device("cuda", 0)


def atrium_model(open_roof):
    text = scene_gen.atrium(1.0)[0]
    line = re.search(r'LightSource "point"[^\n]*\n', text).group(0)
    text = text.replace(line, DISTANT)
    if open_roof:
        roofs = [m.group(0) for m in re.finditer(r'Shape "trianglemesh" "integer indices" \[[^\]]*\] "point P" \[([^\]]*)\]\n', text)
                 if (np.array(m.group(1).split(), np.float64).reshape(-1, 3)[:, 2] == 7.0).all()]
        assert len(roofs) == 1
        text = text.replace(roofs[0], "")
    with tempfile.TemporaryDirectory(prefix="hprt_replay_") as d:      # (the model holds the scene once it is parsed)
        path = os.path.join(d, name + ".pbrt")
        with open(path, "w") as f:
            f.write(text)
        return hprt.Model.parse(path)


model = hprt.Model.load(os.path.join(ROOT, "tests", "golden", "killeroo.hprt")) if name == "killeroo" else atrium_model(name == "atrium-open")
bvh = hprt.Bvh(model)


def make_scene(R):
    os.environ["HPRT_SHADOW_GRID_RES"] = str(R); os.environ["HPRT_SHADOW_GRID"] = "1"      # (a grid whatever its lists' lengths)
    try:
        return hprt.Scene(model, bvh, device=0)
    finally:
        del os.environ["HPRT_SHADOW_GRID_RES"], os.environ["HPRT_SHADOW_GRID"]


scenes = {R: make_scene(R) for R in res}
for R, s in scenes.items():
    info = s.distant_grid_info()
    assert info["eligible"], (name, R)
    print("grid R=%d (asked %d): entries %d, near %d, image %.1f MB, build %.3f s + pack %.3f s, longest list %d, mean %.2f, w %s"
          % (info["R"], R, info["entries"], info["near"], info["bytes"] / 1e6, info["build_seconds"], info["pack_seconds"], info["longest"], info["mean"],
             info["w"]), flush=True)
scene = scenes[res[0]]
opt = model.options.copy(); opt.spp = spp
x0, y0, x1, y1 = opt.film_bounds()
cap = (x1 - x0) * (y1 - y0) * spp
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


for bounce in (0, 1, 2):
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
    print("  k_walk4<any>             %s ms   best %.1f Mrays/s" % (" ".join("%7.3f" % m for m in ms), n / min(ms) / 1e3), flush=True)
    for R, s in scenes.items():
        occ = torch.empty(n, dtype=torch.uint8, device=dev)
        ms = [s.distant_grid_occluded_device(n, rays.data_ptr(), occ.data_ptr()) for _ in range(ITERS + 1)][1:]      # (the kernel alone, as the walk's figure)
        same = bool(torch.equal(occ, occ_walk))
        print("  k_distant_grid R=%-5d   %s ms   best %.1f Mrays/s   answers identical: %s, occluded %.1f %%"
              % (s.distant_grid_info()["R"], " ".join("%7.3f" % m for m in ms), n / min(ms) / 1e3, same, 100.0 * float(occ.float().mean())), flush=True)
        assert same, (name, bounce, R)
        del occ
    del rays, occ_walk
