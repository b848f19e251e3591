"""Rays per second of the two-level kd walk (k_kdinstwalk) beside the BVH walk plain traces of an instanced scene take (k_walk4), on
HBM-resident rays through hprt_intersect_device / hprt_occluded_device.  Scene: the instanced killeroo of tools/scene_gen.py (the
killeroo mesh as one object, 301 instances: instanced-10m).  Ray sets: tools/walk_bench.py's camera rays (closest hit, 700x700 x 4
samples, tile order) and shadow rays from their hit points to a point above the scene's centre (any hit).  Prints one JSON line;
DESIGN.md §8h quotes it.
usage: python tools/bench_kdinst.py [iters]"""
import json, os, sys, tempfile
import walk_bench as wb
from walk_bench import hprt, scene_gen

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 5

d = tempfile.mkdtemp(prefix="hprt_kdinst_")
text, ntri = scene_gen.instanced_killeroo(os.path.join(wb.ROOT, "tests", "golden", "killeroo.hprt"))
open(os.path.join(d, "instanced.pbrt"), "w").write(text)
m = hprt.Model.parse(os.path.join(d, "instanced.pbrt"))
baked = os.path.join(d, "instanced.hprt")
m.save(baked)
bvh_scene = hprt.Scene(m, hprt.Bvh(m), device=0)
kd_scene = hprt.Scene(m, hprt.Bvh(m), device=0)
trees = hprt.KdInst(m)
kd_scene.attach_kdinst(trees)
inf = trees.info()
rays = wb.RaySets(baked, kd_scene)
res = {"instanced_triangles": ntri, "closest_rays": rays.n, "any_rays": rays.ns, "top_nodes": inf["nodes"], "top_depth": inf["depth"],
       "object_nodes": trees.object_info(0)["nodes"], "object_depth": inf["object_depth"], "walk4_in_use": bool(hprt.lib.hprt_debug_scene_walk(bvh_scene._h))}
for label, sc in (("kdinst", kd_scene), ("walk4", bvh_scene)):
    mc = wb.timed(lambda: rays.closest(sc), iters)
    ma = wb.timed(lambda: rays.any(sc), iters)
    res[label + "_closest_grays"] = round(rays.n / mc / 1e6, 3)
    res[label + "_any_grays"] = round(rays.ns / ma / 1e6, 3)
# the two walks answer the same rays the same way up to ties between equally distant hits
t1, p1, _ = bvh_scene.intersect(rays.o, rays.d, rays.inf)
res["closest_same_prim_frac"] = float((p1 == rays.prim).mean())
print(json.dumps({"instanced-killeroo": res}), flush=True)
