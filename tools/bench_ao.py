"""Ambient occlusion (Integrator "ambientocclusion", hprt_render_ao) on killeroo-simple, 700x700 at `spp` samples per pixel and
n_samples = 64 hemisphere rays per hit: the frame time and the any-hit rate on those rays — incoherent, tMax = Infinity, ending at
no light, so never the shadow grid's — through the BVH and through four attached trees: kdtree, rbspkd with 13 directions,
bsppaperkd and bsprandomfastkd with K = 5.  One process: every walk renders once to warm up, then `iters` rounds alternate the walks
and the best frame of each is kept.  Grays/s = shadow_rays / occluded_seconds (HIP events around the any-hit launches), and the share
of the frame spent in k_ao_frame, k_ao_rays and k_ao_resolve comes from HIP events around those launches.  Prints one JSON line per
walk; DESIGN.md §12 quotes them.  No rate is a pass condition.
usage: python tools/bench_ao.py [iters = 5] [spp = 4]"""
import json, sys, time
import walk_bench as wb
from walk_bench import hprt

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 5
spp = int(sys.argv[2]) if len(sys.argv) > 2 else 4
N_SAMPLES = 64

m, _ = wb.scene_model("killeroo-simple")
opt = m.options.copy(); opt.spp = spp
builders = [("bvh", None, None),
            ("kdtree", lambda: hprt.KdTree(m), "attach_kdtree"),
            ("rbspkd-13", lambda: hprt.RbspKd(m, n_directions=13, threads=16), "attach_rbspkd"),
            ("bsppaperkd", lambda: hprt.BspPaperKd(m, isect_cost=80, threads=16), "attach_bsppaperkd"),
            ("bsprandomfastkd-5", lambda: hprt.BspNodeKd(m, "bsprandomfastkd", n_directions=5), "attach_bsppaperkd")]
walks = []
for label, build, attach in builders:
    sc = hprt.Scene(m, hprt.Bvh(m), device=0)
    build_s = 0.0
    if build:
        t0 = time.time(); tree = build(); build_s = time.time() - t0
        getattr(sc, attach)(tree)
    walks.append({"walk": label, "scene": sc, "build_s": round(build_s, 2), "best": None})
    print(json.dumps({"walk": label, "build_s": round(build_s, 2)}), flush=True)


def frame(w):
    _, st = w["scene"].render_ao(N_SAMPLES, True, opt)
    return st, w["scene"].ao_kernel_seconds()


for w in walks:                        # warm-up
    frame(w)
for _ in range(iters):                 # the walks alternated
    for w in walks:
        st, k = frame(w)
        if w["best"] is None or st["render_seconds"] < w["best"][0]["render_seconds"]:
            w["best"] = (st, k)
for w in walks:
    st, k = w["best"]
    f = st["render_seconds"]
    print(json.dumps({"scene": "killeroo-simple", "walk": w["walk"], "spp": spp, "n_samples": N_SAMPLES, "build_s": w["build_s"],
                      "frame_ms": round(f * 1e3, 2), "camera_rays": int(st["camera_rays"]), "ao_rays": int(st["shadow_rays"]),
                      "any_hit_ms": round(st["occluded_seconds"] * 1e3, 2), "any_hit_grays": round(st["shadow_rays"] / st["occluded_seconds"] / 1e9, 3),
                      "closest_hit_ms": round(st["extend_seconds"] * 1e3, 2),
                      "k_ao_frame_ms": round(k[0] * 1e3, 3), "k_ao_rays_ms": round(k[1] * 1e3, 3), "k_ao_resolve_ms": round(k[2] * 1e3, 3),
                      "ao_kernels_share": round(sum(k) / f, 4)}), flush=True)
