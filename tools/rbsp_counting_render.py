"""One counting render of killeroo-simple as its scene file sets it (700x700, 8 spp, maxdepth 5) for the kd-tree and for each
rbsp-N: node traversals (closest / any hit) and primitive tests, the totals DESIGN.md §8b sets beside the thesis table.
usage: python tools/rbsp_counting_render.py"""
import importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
hprt = importlib.import_module("thesis-pbrt-v3_amd")

m = hprt.Model.load(os.path.join(ROOT, "tests", "golden", "killeroo_simple.hprt"))
opt = m.options.copy()
opt.spp = 8
for label, tree in [("kd", lambda: hprt.KdTree(m))] + [("rbsp-%d" % M, (lambda M=M: hprt.Rbsp(m, n_directions=M))) for M in (3, 7, 9, 13)]:
    sc = hprt.Scene(m, hprt.Bvh(m), device=0)
    t = tree()
    (sc.attach_kdtree if label == "kd" else sc.attach_rbsp)(t)
    _, st = sc.render(opt, count_work=True)
    keys = ("rays", "shadow_rays", "nodes_fetched", "nodes_fetched_p", "nodes_entered", "nodes_entered_p", "tri_tests", "tri_tests_p",
            "sphere_tests", "sphere_tests_p")
    print(json.dumps({"tree": label, **{k: int(st[k]) for k in keys}}), flush=True)
