"""Rays per second of the two-level RBSP walk (k_rbspinstwalk) at M = 3 and 13, plain and kd-aware, beside the two-level kd walk
(k_kdinstwalk) and the BVH walk plain traces of an instanced scene take (k_walk4), on HBM-resident rays through
hprt_intersect_device / hprt_occluded_device.  Scene: the instanced killeroo of tools/scene_gen.py (the killeroo mesh as one object,
301 instances: instanced-10m).  Ray sets: tools/walk_bench.py's camera rays (closest hit, 700x700 x 4 samples, tile order) and
shadow rays from their hit points to a point above the scene's centre (any hit).  Every walk is measured warm, in this one process,
on the same ray sets (walk_bench.timed).  Prints one JSON line; DESIGN.md §8j quotes it.
The host builds dominate the run (the killeroo object's tree at M = 13 takes minutes), so the kd-aware trees are measured only
when asked for.
usage: python tools/bench_rbspinst.py [iters] [--kd-aware]"""
import json, os, sys, tempfile, time
import walk_bench as wb
from walk_bench import hprt, scene_gen

args = [a for a in sys.argv[1:] if not a.startswith("--")]
iters = int(args[0]) if args else 5
kinds = (False, True) if "--kd-aware" in sys.argv else (False,)

d = tempfile.mkdtemp(prefix="hprt_rbspinst_")
text, ntri = scene_gen.instanced_killeroo(os.path.join(wb.ROOT, "tests", "golden", "killeroo.hprt"))
open(os.path.join(d, "instanced.pbrt"), "w").write(text)
m = hprt.Model.parse(os.path.join(d, "instanced.pbrt"))
baked = os.path.join(d, "instanced.hprt")
m.save(baked)
bvh_scene = hprt.Scene(m, hprt.Bvh(m), device=0)
scenes = [("walk4", bvh_scene)]
res = {"instanced_triangles": ntri, "walk4_in_use": bool(hprt.lib.hprt_debug_scene_walk(bvh_scene._h))}
t0 = time.perf_counter()
kd_trees = hprt.KdInst(m)
res["kdinst_build_s"] = round(time.perf_counter() - t0, 2)
kd_scene = hprt.Scene(m, hprt.Bvh(m), device=0)
kd_scene.attach_kdinst(kd_trees)
scenes.append(("kdinst", kd_scene))
keep = [kd_trees]
for kd_aware in kinds:
    for M in (3, 13):
        label = ("rbspkdinst%d" if kd_aware else "rbspinst%d") % M
        t0 = time.perf_counter()
        trees = hprt.RbspInst(m, kd_aware=kd_aware, n_directions=M)
        res[label + "_build_s"] = round(time.perf_counter() - t0, 2)
        inf = trees.info()
        res[label + "_trees"] = {"top_nodes": inf["nodes"], "top_depth": inf["depth"], "object_nodes": trees.object_info(0)["nodes"], "object_depth": inf["object_depth"]}
        sc = hprt.Scene(m, hprt.Bvh(m), device=0)
        sc.attach_rbspinst(trees)
        scenes.append((label, sc)); keep.append(trees)
rays = wb.RaySets(baked, kd_scene)
res["closest_rays"], res["any_rays"] = rays.n, rays.ns
for label, sc in scenes:
    mc = wb.timed(lambda: rays.closest(sc), iters)
    ma = wb.timed(lambda: rays.any(sc), iters)
    res[label + "_closest_grays"] = round(rays.n / mc / 1e6, 3)
    res[label + "_any_grays"] = round(rays.ns / ma / 1e6, 3)
# the walks answer the same rays the same way up to ties between equally distant hits
for label, sc in scenes[2:]:
    t1, p1, _ = sc.intersect(rays.o, rays.d, rays.inf)
    res[label + "_same_prim_frac"] = float((p1 == rays.prim).mean())
print(json.dumps({"instanced-killeroo": res}), flush=True)
