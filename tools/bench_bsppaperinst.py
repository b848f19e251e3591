"""Rays per second of the two-level general BSP walk (k_bsppaperinstwalk), plain and kd-aware, beside the two-level RBSP walk at
M = 13 (k_rbspinstwalk), the two-level kd walk (k_kdinstwalk) and the BVH walk plain traces of an instanced scene take (k_walk4), on
HBM-resident rays through hprt_intersect_device / hprt_occluded_device.  Scene: the instanced killeroo of tools/scene_gen.py (the
killeroo mesh as one object, 301 instances: instanced-10m).  Ray sets: tools/walk_bench.py's camera rays (closest hit, 700x700 x 4
samples, tile order) and shadow rays from their hit points to a point above the scene's centre (any hit).  Every walk is measured
warm, in this one process, on the same ray sets (walk_bench.timed: best of `iters`, default 5).  Prints one JSON line with the
Grays/s, every tree's node counts and depths and the host build times; DESIGN.md §8m quotes it.
The host builds dominate the run: the general BSP tree over the killeroo object's 33,264 triangles takes on the order of the 100 s
DESIGN.md §8d records for that mesh, and the RBSP tree at M = 13 about two minutes (§8j) — --no-rbsp leaves that one out.
usage: python tools/bench_bsppaperinst.py [iters] [--no-rbsp]"""
import json, os, sys, tempfile, time
import walk_bench as wb
from walk_bench import hprt, scene_gen

args = [a for a in sys.argv[1:] if not a.startswith("--")]
iters = int(args[0]) if args else 5

d = tempfile.mkdtemp(prefix="hprt_bsppaperinst_")
text, ntri = scene_gen.instanced_killeroo(os.path.join(wb.ROOT, "tests", "golden", "killeroo.hprt"))
open(os.path.join(d, "instanced.pbrt"), "w").write(text)
m = hprt.Model.parse(os.path.join(d, "instanced.pbrt"))
baked = os.path.join(d, "instanced.hprt")
m.save(baked)
bvh_scene = hprt.Scene(m, hprt.Bvh(m), device=0)
scenes = [("walk4", bvh_scene)]
res = {"instanced_triangles": ntri, "walk4_in_use": bool(hprt.lib.hprt_debug_scene_walk(bvh_scene._h))}


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
for kd_aware in (False, True):
    keep.append(add("bsppaperkdinst" if kd_aware else "bsppaperinst", lambda: hprt.BspPaperInst(m, kd_aware=kd_aware, isect_cost=80), "attach_bsppaperinst"))
rays = wb.RaySets(baked, scenes[1][1])
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
