"""Rays per second of the two-level walk (k_bsppaperinstwalk, unchanged) over two-level NODE-BASED trees — "bspclusterfastkd",
"bsprandomfastkd" (KD = true) and "bspcluster" (KD = false) at K = 5 — beside the two-level kd walk (k_kdinstwalk), the two-level
RBSP walk at M = 13 (k_rbspinstwalk), the same kernel over two-level bsppaperkd trees, and the BVH walk plain traces of an instanced
scene take (k_walk4), on HBM-resident rays through hprt_intersect_device / hprt_occluded_device.  Scene: the instanced killeroo of
tools/scene_gen.py (the killeroo mesh as one object, 301 instances).  Ray sets: tools/walk_bench.py's camera rays (closest hit) and
shadow rays from their hit points (any hit).  Every walk is measured warm, in this one process, on the same ray sets
(walk_bench.timed: best of `iters`, default 5).  Each node-based handle is built twice in this process: on the host
(hprt_bspnodeinst_build, 16 threads) and device-assisted (hprt_bspnodeinst_build_device, one session for both trees); the seconds
of the second are to be compared with the seconds of the first and with nothing else, and the two handles must hold the same bytes.
Prints one JSON line with the Grays/s, every tree's node counts and depths, and the build times; DESIGN.md §8r quotes it.
The host builds dominate the run (minutes per tree over the object's 33,264 triangles); --no-rbsp and --no-bsppaperkd leave the
comparison trees out, --no-device the device-assisted builds.
usage: python tools/bench_bspnodeinst.py [iters] [--no-rbsp] [--no-bsppaperkd] [--no-device]"""
import json, os, sys, tempfile, time
import walk_bench as wb
from walk_bench import hprt, scene_gen

args = [a for a in sys.argv[1:] if not a.startswith("--")]
iters = int(args[0]) if args else 5
K, SEED = 5, hprt.BSPNODE_DEFAULT_SEED
NODE_BASED = ("bspclusterfastkd", "bsprandomfastkd", "bspcluster")

d = tempfile.mkdtemp(prefix="hprt_bspnodeinst_")
text, ntri = scene_gen.instanced_killeroo(os.path.join(wb.ROOT, "tests", "golden", "killeroo.hprt"))
open(os.path.join(d, "instanced.pbrt"), "w").write(text)
m = hprt.Model.parse(os.path.join(d, "instanced.pbrt"))
baked = os.path.join(d, "instanced.hprt")
m.save(baked)
bvh_scene = hprt.Scene(m, hprt.Bvh(m), device=0)
scenes = [("walk4", bvh_scene)]
res = {"instanced_triangles": ntri, "K": K, "seed": SEED, "walk4_in_use": bool(hprt.lib.hprt_debug_scene_walk(bvh_scene._h))}


def add(label, build, attach):
    """build the trees on the host (timed), attach them to a scene of their own"""
    t0 = time.perf_counter()
    trees = build()
    res[label + "_build_s"] = round(time.perf_counter() - t0, 2)
    inf = trees.info()
    res[label + "_trees"] = {"top_nodes": inf["nodes"], "top_depth": inf["depth"], "object_nodes": trees.object_info(0)["nodes"], "object_depth": inf["object_depth"]}
    for k in ("axis_interior", "plane_interior"):
        if k in inf:
            res[label + "_trees"][k] = inf[k]
    sc = hprt.Scene(m, hprt.Bvh(m), device=0)
    getattr(sc, attach)(trees)
    scenes.append((label, sc))
    return trees


keep = [add("kdinst", lambda: hprt.KdInst(m), "attach_kdinst")]
if "--no-rbsp" not in sys.argv:
    keep.append(add("rbspinst13", lambda: hprt.RbspInst(m, kd_aware=False, n_directions=13), "attach_rbspinst"))
if "--no-bsppaperkd" not in sys.argv:
    keep.append(add("bsppaperkdinst", lambda: hprt.BspPaperInst(m, kd_aware=True, isect_cost=80), "attach_bsppaperinst"))
for acc in NODE_BASED:
    host = add(acc + "inst", lambda: hprt.BspNodeInst(m, acc, n_directions=K, seed=SEED), "attach_bsppaperinst")
    keep.append(host)
    if "--no-device" not in sys.argv:
        t0 = time.perf_counter()
        dev = hprt.BspNodeInst(m, acc, n_directions=K, seed=SEED, device=0)
        res[acc + "inst_build_device_s"] = round(time.perf_counter() - t0, 2)
        res[acc + "inst_build_device_stats"] = dev.build_stats
        res[acc + "inst_device_same_bytes"] = all(a.tobytes() == b.tobytes() for x, y in ((host.copy(), dev.copy()), (host.object_copy(0), dev.object_copy(0)))
                                                  for a, b in zip(x, y))
rays = wb.RaySets(baked, scenes[1][1])
res["closest_rays"], res["any_rays"] = rays.n, rays.ns
for label, sc in scenes:
    mc = wb.timed(lambda: rays.closest(sc), iters)
    ma = wb.timed(lambda: rays.any(sc), iters)
    res[label + "_closest_grays"] = round(rays.n / mc / 1e6, 3)
    res[label + "_any_grays"] = round(rays.ns / ma / 1e6, 3)
# the walks answer the same rays the same way up to ties between equally distant hits — and, for the cluster trees, up to the hits a
# triangle lying in its own split plane loses
for label, sc in scenes[2:]:
    t1, p1, _ = sc.intersect(rays.o, rays.d, rays.inf)
    res[label + "_same_prim_frac"] = float((p1 == rays.prim).mean())
print(json.dumps({"instanced-killeroo": res}), flush=True)
