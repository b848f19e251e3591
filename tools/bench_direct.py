"""Direct lighting (Integrator "directlighting", hprt_render_direct) on killeroo-simple, 700x700 at `spp` samples per pixel, strategy
"all", maxdepth 5, at two settings of the light's sample count: the scene's own (its AreaLightSource line says "nsamples" 8; the
baked fixture keeps no counts, so the figure stands here) and 16.  The frame time, and the any-hit rate on the light-directed shadow
rays and the closest-hit rate on the node rays and EstimateDirect's BSDF-sampled rays, through the BVH and through four attached
trees: kdtree, rbspkd with 13 directions, bsppaperkd and bsprandomfastkd with K = 5 — the walks of tools/bench_ao.py.  One process:
every (walk, setting) renders once to warm up, then `iters` rounds alternate them and the best frame of each is kept.  Rates =
rays / seconds of HIP events around the trace launches; the share of the frame spent in k_dl_shade, k_dl_rays, k_dl_resolve and
k_dl_advance comes from HIP events around those launches.  Prints one JSON line per walk and setting; DESIGN.md §13 quotes them.
No rate is a pass condition.
usage: python tools/bench_direct.py [iters = 5] [spp = 4]"""
import json, sys, time
import walk_bench as wb
from walk_bench import hprt

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 5
spp = int(sys.argv[2]) if len(sys.argv) > 2 else 4
MAX_DEPTH = 5
OWN = 8      # "integer nsamples" [8] of the scene's AreaLightSource "area" line

m, _ = wb.scene_model("killeroo-simple")
n_lights = m.counts()["lights"]
opt = m.options.copy(); opt.spp = spp
builders = [("bvh", None, None),
            ("kdtree", lambda: hprt.KdTree(m), "attach_kdtree"),
            ("rbspkd-13", lambda: hprt.RbspKd(m, n_directions=13, threads=16), "attach_rbspkd"),
            ("bsppaperkd", lambda: hprt.BspPaperKd(m, isect_cost=80, threads=16), "attach_bsppaperkd"),
            ("bsprandomfastkd-5", lambda: hprt.BspNodeKd(m, "bsprandomfastkd", n_directions=5), "attach_bsppaperkd")]
runs = []
for label, build, attach in builders:
    sc = hprt.Scene(m, hprt.Bvh(m), device=0)
    build_s = 0.0
    if build:
        t0 = time.time(); tree = build(); build_s = time.time() - t0
        getattr(sc, attach)(tree)
    for n in (OWN, 16):
        runs.append({"walk": label, "n": n, "scene": sc, "build_s": round(build_s, 2), "best": None})
    print(json.dumps({"walk": label, "build_s": round(build_s, 2)}), flush=True)


def frame(r):
    _, st = r["scene"].render_direct("all", MAX_DEPTH, [r["n"]] * n_lights, opt=opt)
    return st, r["scene"].dl_kernel_seconds()


for r in runs:                         # warm-up
    frame(r)
for _ in range(iters):                 # the walks and settings alternated
    for r in runs:
        st, k = frame(r)
        if r["best"] is None or st["render_seconds"] < r["best"][0]["render_seconds"]:
            r["best"] = (st, k)
for r in runs:
    st, (k, steps) = r["best"]
    f = st["render_seconds"]
    print(json.dumps({"scene": "killeroo-simple", "walk": r["walk"], "spp": spp, "strategy": "all", "maxdepth": MAX_DEPTH, "light_samples": r["n"],
                      "build_s": r["build_s"], "frame_ms": round(f * 1e3, 2), "steps": steps, "camera_rays": int(st["camera_rays"]),
                      "closest_hit_rays": int(st["rays"]), "shadow_rays": int(st["shadow_rays"]),
                      "any_hit_ms": round(st["occluded_seconds"] * 1e3, 2), "any_hit_grays": round(st["shadow_rays"] / max(st["occluded_seconds"], 1e-12) / 1e9, 3),
                      "closest_hit_ms": round(st["extend_seconds"] * 1e3, 2), "closest_hit_grays": round(st["rays"] / max(st["extend_seconds"], 1e-12) / 1e9, 3),
                      "k_dl_shade_ms": round(k[0] * 1e3, 3), "k_dl_rays_ms": round(k[1] * 1e3, 3), "k_dl_resolve_ms": round(k[2] * 1e3, 3),
                      "k_dl_advance_ms": round(k[3] * 1e3, 3), "dl_kernels_share": round(sum(k) / f, 4)}), flush=True)
