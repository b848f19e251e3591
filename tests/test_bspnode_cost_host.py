"""bspnode_cost.h on the host: the fixed-capacity restatement of one node-based BSP split candidate (per direction: DirectionId, its
place in the compact table; per candidate: the cut, the two surface areas over the child's directions and the formula of the
direction's kind) against the builder's vector code, bit for bit, on the candidates of real build nodes (handed out by the builder
itself); the odd direction sets; the flags at the compiled and at lowered capacities; a sweep beyond the direction table; the
validation of the diagnostics hook; the device entries without a device; a stand-alone sanitizer run of the header.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bspnode_cost_nodes as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def agree(hprt, nd, impl, cands=None, **over):
    """costs nd with impl; asserts that every unflagged candidate carries impl 0's cost and fixed cost; returns the flags"""
    rc0, c0, f0, o0, d0 = B.cost(hprt, nd, 0, cands=cands, **{k: v for k, v in over.items() if k not in B.CAPS})
    rc, c, f, o, d = B.cost(hprt, nd, impl, cands=cands, **over)
    assert rc0 == 0 and rc == 0 and d0 == 0 and not o0.any() and set(np.unique(o)) <= {0, 1}
    if d:
        assert o.all()
    ok = o == 0
    assert B.equal_where(ok, c, c0) and B.equal_where(ok, f, f0)
    return o


@pytest.mark.parametrize("key", B.node_sets(), ids=B.set_id)
def test_restatement_equals_the_vector_code(hprt, key):
    """impl 1 == impl 0 == the costs and fixed costs the builder's own costRange gave, on every candidate of the first 64 costed
    nodes; no flag is set at the compiled capacities, so nothing here (or in the GPU tests) passes by falling back"""
    nodes = B.nodes_of(key)
    assert 1 <= len(nodes) <= B.NODES
    sizes, chosen = [], 0
    for nd in nodes:
        bc, bf = B.builder_results(nd)
        rc0, c0, f0, o0, d0 = B.cost(hprt, nd, 0)
        rc1, c1, f1, o1, d1 = B.cost(hprt, nd, 1)
        assert rc0 == 0 and rc1 == 0 and d0 == 0 and d1 == 0 and not o0.any() and not o1.any()
        assert B.same_bits(c0, bc) and B.same_bits(f0, bf)
        assert B.same_bits(c1, c0) and B.same_bits(f1, f0)
        kinds = nd["sweep"]["kind"][nd["cands"]["k"]]
        assert set(np.unique(nd["sweep"]["kind"])) <= ({B.KD_AXIS, B.CHOSEN} if nd["fastkd"] else {B.PLAIN})
        assert np.isposinf(f0[kinds != B.CHOSEN]).all() and np.isfinite(f0[kinds == B.CHOSEN]).all()
        assert (np.diff(nd["cands"]["k"].astype(np.int64)) >= 0).all()      # (direction, edge) order
        sizes.append(len(c0)); chosen += int((kinds == B.CHOSEN).sum())
    assert max(sizes) > 64 and sum(sizes) > 1000
    assert (chosen > 0) == key[1].endswith("fastkd")


def deep_nodes(hprt, name, K=4):
    nodes = B.build_nodes(hprt, name, K, p9=dict(B.soups(300))["grid1"], max_nodes=400)
    return [nd for nd in nodes if nd["level"] >= 8 and len(nd["dirs"]) > 9]


def faceless_direction_nodes(nodes, limit=12):
    """nodes made from deep ones: the first sweep direction is replaced by one of the node's OWN directions that owns no face of
    its mesh (an ancestor's split the mesh no longer touches), once exactly and once tilted by a quarter of a degree, with
    candidates spread over the mesh's extent along it.  Such a direction takes the node's id (below M), its faces enter the compact
    table between the others, and the areas are measured along the node's vector, not the sweep's."""
    out = []
    for nd in nodes:
        dirs = nd["dirs"].reshape(-1, 3)
        owners = set((nd["edges"]["f1"] // 2).tolist()) | set((nd["edges"]["f2"] // 2).tolist())
        free = [d for d in range(len(dirs) - 1) if d not in owners and d < max(owners)]
        if not free or len(nd["edges"]) == 0:
            continue
        own = dirs[free[len(free) // 2]]
        tilt = own.astype(np.float64) + 0.004 * np.roll(own.astype(np.float64), 1)
        tilt = (tilt / np.linalg.norm(tilt)).astype(np.float32)
        for axis in (own, tilt):
            if float(axis.astype(np.float64) @ own.astype(np.float64)) <= 0.99997:
                continue
            sweep = nd["sweep"].copy()
            sweep["axis"][0] = axis
            pts = np.concatenate([nd["edges"]["v1"], nd["edges"]["v2"]]).astype(np.float64) @ axis.astype(np.float64)
            ts = np.linspace(pts.min(), pts.max(), 23)[1:-1].astype(np.float32)
            cands = np.zeros(len(ts), B.CAND)
            cands["k"] = 0; cands["t"] = ts; cands["nBelow"] = np.arange(len(ts)); cands["nAbove"] = len(ts) - 1 - np.arange(len(ts))
            out.append(dict(nd, sweep=sweep, cands=np.concatenate([cands, nd["cands"][nd["cands"]["k"] > 0]])))
        if len(out) >= limit:
            break
    return out


@pytest.mark.parametrize("name", ("bsprandom", "bspclusterwithkd", "bsparbitraryfastkd"))
def test_deep_nodes_with_grown_direction_lists(hprt, name):
    """nodes at least 8 levels below the root whose direction list has grown past the three axes: the compaction of the faces and
    a direction entering the table in the middle or at the end"""
    deep = deep_nodes(hprt, name)
    assert deep and max(len(nd["dirs"]) // 3 for nd in deep) > 6
    for nd in deep[:48]:
        assert not agree(hprt, nd, 1).any()


def test_a_sweep_direction_that_owns_no_face_keeps_the_nodes_vector(hprt):
    made = faceless_direction_nodes(deep_nodes(hprt, "bsprandom") + deep_nodes(hprt, "bsprandomfastkd"))
    assert len(made) >= 4
    moved = 0
    for nd in made:
        assert not agree(hprt, nd, 1).any()
        # the node's direction did take the candidates: along a direction of its own (new to the node) they cost something else
        own = nd["sweep"]["axis"][0]
        other = nd["sweep"].copy(); other["axis"][0] = (own + np.float32(0.05) * np.roll(own, 1)) / np.linalg.norm(own + np.float32(0.05) * np.roll(own, 1))
        first = nd["cands"]["k"] == 0
        moved += int((B.cost(hprt, nd, 0, sweep=other)[1].view(np.uint32)[first] != B.cost(hprt, nd, 0)[1].view(np.uint32)[first]).sum())
    assert moved > 0


def odd_direction_sets(hprt, tmp_path):
    """{label: nodes}: fastkd with K = 3 (no chosen direction), plain with K = 1, nodes with np <= K under cluster and arbitrary
    (fewer sweep directions than K), two equal sweep directions, a zero and a NaN direction, spheres among triangles"""
    p9 = dict(B.soups(200))["random"]
    out = {}
    out["fastkd-K3"] = B.build_nodes(hprt, "bspclusterfastkd", 3, p9=p9, max_nodes=24)
    assert all(len(nd["sweep"]) == 3 and (nd["sweep"]["kind"] == B.KD_AXIS).all() for nd in out["fastkd-K3"])
    out["plain-K1"] = B.build_nodes(hprt, "bsprandom", 1, p9=p9, max_nodes=24)
    assert all(len(nd["sweep"]) == 1 for nd in out["plain-K1"])
    for name in ("bspcluster", "bsparbitrary"):
        few = [nd for nd in B.build_nodes(hprt, name, 6, p9=p9, max_nodes=200) if len(nd["sweep"]) < 6]
        assert few, name
        out[name + "-np<=K"] = few[:24]
    # the dodecahedron's pentagons are three coplanar triangles each: their normals are equal sweep directions
    equal = [nd for nd in B.build_nodes(hprt, "bsparbitrary", 6, model=hprt.Model.load(B.DODECA), max_nodes=200)
             if len(np.unique(nd["sweep"]["axis"], axis=0)) < len(nd["sweep"])]
    nd = B.nodes_of(((200, "random"), "bsprandom", 4))[0]
    twice = dict(nd, sweep=np.concatenate([nd["sweep"], nd["sweep"][1:2]]),
                 cands=np.concatenate([nd["cands"], np.array([(len(nd["sweep"]),) + tuple(c)[1:] for c in nd["cands"][nd["cands"]["k"] == 1]], B.CAND)]))
    out["equal-directions"] = equal[:12] + [twice]
    assert len(np.unique(twice["sweep"]["axis"], axis=0)) < len(twice["sweep"])
    zero = nd["sweep"].copy(); zero["axis"][2] = 0            # a direction that yields no candidate: nothing refers to it
    nan = nd["sweep"].copy(); nan["axis"][2] = np.nan
    out["zero-direction"] = [dict(nd, sweep=zero, cands=nd["cands"][nd["cands"]["k"] != 2]), dict(nd, sweep=nan, cands=nd["cands"][nd["cands"]["k"] != 2])]
    out["spheres"] = sphere_nodes(hprt, tmp_path)
    return out


def sphere_model(hprt, tmp_path):
    from test_host_side import HEADER
    rng = np.random.default_rng(4)
    spheres = "".join('AttributeBegin Translate %r %r %r Shape "sphere" "float radius" [%r] AttributeEnd\n' % (*map(float, rng.uniform(-3, 3, 3)), float(rng.uniform(0.2, 0.9)))
                      for _ in range(12))
    p9 = dict(B.soups(200))["random"][:60] * np.float32(0.3)
    tris = 'Shape "trianglemesh" "integer indices" [%s] "point P" [%s]\n' % (" ".join(map(str, range(180))), " ".join(repr(float(v)) for v in p9.ravel()))
    (tmp_path / "s.pbrt").write_text(HEADER + spheres + tris + "WorldEnd\n")
    return hprt.Model.parse(str(tmp_path / "s.pbrt"))


def sphere_nodes(hprt, tmp_path):
    """spheres among triangles: a sphere has no normal, so the choosers hand out the direction PositiveX makes of (0, 0, 0)"""
    m = sphere_model(hprt, tmp_path)
    return B.build_nodes(hprt, "bspcluster", 4, model=m, max_nodes=16) + B.build_nodes(hprt, "bsparbitraryfastkd", 5, model=m, max_nodes=16)


def test_odd_direction_sets(hprt, tmp_path):
    sets = odd_direction_sets(hprt, tmp_path)
    for label, nodes in sets.items():
        assert nodes, label
        for nd in nodes:
            assert not agree(hprt, nd, 1).any(), label
    tw = sets["equal-directions"][-1]
    c = B.cost(hprt, tw, 1)[1]
    assert B.same_bits(c[tw["cands"]["k"] == 1], c[tw["cands"]["k"] == len(tw["sweep"]) - 1])


LOWERED = (("maxEdges", 16), ("maxFaces", 10), ("maxFaceEdges", 5))
LOWERED_SETS = (((300, "grid1"), "bsprandom", 4), ((200, "random"), "bspclusterfastkd", 6))


@pytest.mark.parametrize("field,value", LOWERED, ids=[f for f, _ in LOWERED])
def test_lowered_capacity_flags_and_never_lies(hprt, field, value):
    """each capacity lowered until some candidates are flagged; an unflagged one carries the vector code's cost"""
    flagged = clean = 0
    for key in LOWERED_SETS:
        for nd in B.nodes_of(key):
            o = agree(hprt, nd, 1, **{field: value})
            if field == "maxEdges" and len(nd["edges"]) > value:
                assert o.all()      # a node's mesh beyond the capacity is declined whole
            flagged += int(o.sum()); clean += int((o == 0).sum())
    assert flagged > 0 and clean > 0


def test_more_sweep_directions_than_the_table_holds_is_declined(hprt):
    nodes = B.build_nodes(hprt, "bsprandom", B.MAX_SWEEP_DIRS + 1, p9=dict(B.soups(200))["random"][:40], max_nodes=4)
    assert nodes and all(len(nd["sweep"]) == B.MAX_SWEEP_DIRS + 1 for nd in nodes)
    for nd in nodes:
        rc0, c0, f0, o0, d0 = B.cost(hprt, nd, 0)
        rc1, c1, f1, o1, d1 = B.cost(hprt, nd, 1)
        assert rc0 == 0 and d0 == 0 and not o0.any() and B.same_bits(c0, nd["costs"])
        assert rc1 == 0 and d1 == 1 and o1.all()
        # one direction fewer fits
        keep = nd["cands"]["k"] < B.MAX_SWEEP_DIRS
        assert not agree(hprt, nd, 1, cands=nd["cands"][keep], sweep=nd["sweep"][:B.MAX_SWEEP_DIRS]).any()


def test_debug_hook_rejects_malformed_input(hprt):
    nd = B.nodes_of(((200, "random"), "bspclusterfastkd", 4))[0]
    E = hprt.E_INVALID
    for impl in (0, 1):
        assert B.cost(hprt, nd, impl)[0] == 0
        assert B.cost(hprt, nd, impl, M=0)[0] == E
        bad = nd["edges"].copy(); bad["f1"][3] = 2 * (len(nd["dirs"]) // 3)
        assert B.cost(hprt, nd, impl, edges=bad)[0] == E
        bad = nd["edges"].copy(); bad["f2"][0] = 0xffffffff
        assert B.cost(hprt, nd, impl, edges=bad)[0] == E
        bad = nd["cands"].copy(); bad["k"][0] = len(nd["sweep"])             # a direction the sweep does not have
        assert B.cost(hprt, nd, impl, cands=bad)[0] == E
        bad = nd["cands"].copy(); bad["k"][-1] = 0xffffffff
        assert B.cost(hprt, nd, impl, cands=bad)[0] == E
        bad = nd["sweep"].copy(); bad["kind"][0] = 3                         # no such formula
        assert B.cost(hprt, nd, impl, sweep=bad)[0] == E
        bad = nd["sweep"].copy(); bad["kind"][0] = B.PLAIN                   # a plain direction in a fastkd node
        assert B.cost(hprt, nd, impl, sweep=bad)[0] == E
        assert B.cost(hprt, nd, impl, fastkd=False)[0] == E                  # fastkd kinds in a plain node
        assert B.cost(hprt, nd, impl, sweep=nd["sweep"][:0])[0] == E
        for f in B.CAPS:
            assert B.cost(hprt, nd, impl, **{f: 4096})[0] == E               # may only lower the capacity
    assert B.cost(hprt, nd, 3)[0] == E and B.cost(hprt, nd, -1)[0] == E
    assert hprt.lib.hprt_debug_bspnode_cost(None, 0, 1, None, None, None, None) == E
    # a mesh of more edges than the capacity: valid input, the node is declined whole, nothing costed
    big = np.concatenate([nd["edges"]] * 12)
    assert len(big) > 64
    rc, c, f, o, d = B.cost(hprt, nd, 1, edges=big)
    assert rc == 0 and d == 1 and o.all()


def test_device_entries_without_a_device(hprt):
    """hprt_bspnode*_build*_device: HPRT_E_NO_DEVICE and *out NULL where there is no HIP device; the host's argument checks and
    the refusal of instanced models come first"""
    import torch
    p9 = dict(B.soups(200))["random"][:50]
    vp = p9.ctypes.data_as(C.c_void_p)
    m = hprt.Model.load(B.DODECA)
    plain, fast = B.params(hprt, "bspcluster", 4), B.params(hprt, "bspclusterfastkd", 4)
    calls = (("hprt_bspnode_build_from_triangles_device", (p9.shape[0], vp), plain), ("hprt_bspnodekd_build_from_triangles_device", (p9.shape[0], vp), fast),
             ("hprt_bspnode_build_device", (m._h,), plain), ("hprt_bspnodekd_build_device", (m._h,), fast))
    for name, head, q in calls:
        h = C.c_void_p(0xdead)
        st = hprt.BuildDeviceStats()
        rc = getattr(hprt.lib, name)(*head, C.byref(q), None, C.byref(st), C.byref(h))
        if torch.cuda.is_available():
            assert rc == 0 and h.value
            (hprt.lib.hprt_bsppaperkd_destroy if "kd_" in name else hprt.lib.hprt_bsppaper_destroy)(h)
        else:
            assert rc == hprt.E_NO_DEVICE and h.value is None, name
    if not torch.cuda.is_available():
        for cls, acc in ((hprt.BspNode, "bsprandom"), (hprt.BspNodeKd, "bsprandomfastkd")):
            with pytest.raises(hprt.HprtError) as e:
                cls(m, acc, n_directions=4, device=0)
            assert e.value.code == hprt.E_NO_DEVICE
            with pytest.raises(hprt.HprtError) as e:
                cls.from_triangles(p9, acc, n_directions=4, device=0, min_candidates=1)
            assert e.value.code == hprt.E_NO_DEVICE
        with pytest.raises(hprt.HprtError) as e:
            hprt.bspnode_tree(m, "bspclusterfastkd", n_directions=4, device=0, min_candidates=1)
        assert e.value.code == hprt.E_NO_DEVICE
    inst = hprt.Model.load(os.path.join(os.path.dirname(B.DODECA), "simple_instanced.hprt"))
    for name, q in (("hprt_bspnode_build_device", plain), ("hprt_bspnodekd_build_device", fast)):
        h = C.c_void_p(0xdead)
        assert getattr(hprt.lib, name)(inst._h, C.byref(q), None, None, C.byref(h)) == hprt.E_UNSUPPORTED and h.value is None
    # what the builder refuses from the parameters alone is refused with the host entry's code and message, with or without a device
    for name, host, acc in (("hprt_bspnode_build_from_triangles_device", "hprt_bspnode_build_from_triangles", "bspclusterwithkd"),
                            ("hprt_bspnodekd_build_from_triangles_device", "hprt_bspnodekd_build_from_triangles", "bsprandomfastkd")):
        q = B.params(hprt, acc, 2)
        h = C.c_void_p(0xdead)
        assert getattr(hprt.lib, host)(p9.shape[0], vp, C.byref(q), C.byref(h)) == hprt.E_UNSUPPORTED
        said = hprt.lib.hprt_last_error()
        h = C.c_void_p(0xdead)
        assert getattr(hprt.lib, name)(p9.shape[0], vp, C.byref(q), None, None, C.byref(h)) == hprt.E_UNSUPPORTED and h.value is None
        assert hprt.lib.hprt_last_error() == said and b"nbDirections 2" in said
    h = C.c_void_p(0xdead)      # the wrong form for the handle
    assert hprt.lib.hprt_bspnode_build_device(m._h, C.byref(fast), None, None, C.byref(h)) == hprt.E_INVALID and h.value is None
    assert hprt.BspNode(m, "bspcluster", n_directions=4).build_stats is None       # the host build keeps no device statistics
    assert hprt.BspNodeKd.from_triangles(p9, "bspclusterfastkd", n_directions=4).build_stats is None


SANITIZER_DRIVER = r"""
// bspnode_cost.h on real nodes of node-based builds, at the compiled and at lowered capacities, against the builder's vector code;
// built with -fsanitize=address,undefined and run on its own
#include <cstdio>
#include <cstring>
#include <vector>
#include "bspnode_builder.h"
using namespace hprt;
using namespace hprt::bspnodecost;
static uint32_t rng = 12345u;
static float uni() { rng = rng * 1664525u + 1013904223u; return (float)(rng >> 8) / 16777216.0f; }
int main() {
    const size_t n = 60;
    std::vector<float> p9(9 * n), lo(3 * n), hi(3 * n);
    for (size_t i = 0; i < n; ++i) {
        const float c[3] = {20 * uni() - 10, 20 * uni() - 10, 20 * uni() - 10};
        for (int v = 0; v < 3; ++v) for (int d = 0; d < 3; ++d) p9[9 * i + 3 * v + d] = (float)(int)(c[d] + 4 * uni() - 2);
        for (int d = 0; d < 3; ++d) {
            float a = p9[9 * i + d], b = a;
            for (int v = 1; v < 3; ++v) { const float x = p9[9 * i + 3 * v + d]; a = x < a ? x : a; b = x > b ? x : b; }
            lo[3 * i + d] = a; hi[3 * i + d] = b;
        }
    }
    std::vector<uint8_t> isTri(n, 1);
    isTri[7] = 0; isTri[23] = 0;                       // two primitives without a normal
    int fails = 0; size_t nodes = 0, flagged = 0, costed = 0;
    const int forms[4][3] = {{BSPNODE_RANDOM, BSPNODE_PLAIN, 4}, {BSPNODE_CLUSTER, BSPNODE_FASTKD, 5}, {BSPNODE_ARBITRARY, BSPNODE_WITHKD, 6},
                             {BSPNODE_RANDOM, BSPNODE_FASTKD, 3}};
    for (const auto &form : forms) {
        size_t seen = 0;
        BspNodeParams p; p.chooser = form[0]; p.form = form[1]; p.nDirections = form[2]; p.threads = 1; p.costMinCandidates = 1;
        p.costFn = [&](const BspNodeCostRequest &rq, std::string *) -> int {
            if (seen >= 30) return 1;
            ++seen; ++nodes;
            std::vector<float> c0(rq.n), f0(rq.n);
            std::vector<uint8_t> o0(rq.n);
            BspNodeCostRequest v = rq; v.costs = c0.data(); v.costsFixed = rq.fastKd ? f0.data() : nullptr; v.overflow = o0.data();
            BspNodeCostVector(v);
            const uint32_t lowered[3][3] = {{0, 0, 0}, {16, 10, 5}, {24, 8, 6}};
            for (const auto &low : lowered) {
                bspcost::Scalars sc = rq.sc; sc.maxEdges = low[0]; sc.maxFaces = low[1]; sc.maxFaceEdges = low[2];
                uint32_t cap[4];
                if (!bspcost::Capacities(sc, cap)) { ++fails; continue; }
                if (rq.nEdges > cap[0] || rq.M > BSP_MAX_DIRS || rq.nDirs > BSPNODE_MAX_SWEEP_DIRS) continue;
                std::vector<Edge> mesh(rq.nEdges); std::vector<uint32_t> cdir(rq.M); uint32_t nD = 0;
                bspcost::CompactNode(rq.mesh, rq.nEdges, rq.M, mesh.data(), cdir.data(), &nD);
                if (2 * nD > cap[1]) continue;
                // exactly the capacity's storage, so that a write past it is a heap overflow the sanitizer sees
                std::vector<Q> words(4 * (size_t)cap[0] + 2 * (size_t)cap[1]);
                std::vector<uint8_t> list(cap[2]), o(rq.n);
                std::vector<float> c(rq.n), f(rq.n);
                CostNode(mesh.data(), rq.nEdges, rq.dirs, rq.M, cdir.data(), nD, rq.fastKd, sc, rq.sweep, rq.nDirs, rq.cands, rq.n, cap, words.data(),
                         list.data(), c.data(), f.data(), o.data());
                for (size_t k = 0; k < rq.n; ++k) {
                    ++costed;
                    if (o[k]) { ++flagged; if (!low[0]) ++fails; continue; }
                    if (std::memcmp(&c[k], &c0[k], 4)) ++fails;
                    if (rq.fastKd && std::memcmp(&f[k], &f0[k], 4)) ++fails;
                }
            }
            return 1;      // the build itself goes on with its own code
        };
        BspPaperTree t;
        const std::string err = BuildBspNodeTree(n, lo.data(), hi.data(), p9.data(), isTri.data(), p, &t);
        if (!err.empty()) { std::printf("build: %s\n", err.c_str()); ++fails; }
    }
    std::printf("nodes %zu candidates %zu flagged %zu fails %d\n", nodes, costed, flagged, fails);
    return (fails == 0 && nodes >= 100 && flagged > 0 && costed > flagged) ? 0 : 1;
}
"""


def test_header_runs_clean_under_the_sanitizers(tmp_path):
    """a stand-alone program with its own main over bspnode_cost.h, built with -fsanitize=address,undefined and run directly: the
    storage is sized to the capacity in force, so a write past it would be reported"""
    src = tmp_path / "bspnode_cost_san.cpp"
    src.write_text(SANITIZER_DRIVER)
    csrc = os.path.join(ROOT, "thesis-pbrt-v3_amd", "csrc")
    exe = str(tmp_path / "bspnode_cost_san")
    common = ["g++", "-std=c++17", "-Wall", "-Werror", "-pthread", "-ffp-contract=off", "-fno-fast-math", "-I" + csrc]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # the driver, and with it every instantiation of the header it drives, is built under the sanitizers; the builder that hands
    # out the nodes is the library's own source, built plainly beside it with what it links to (four compilers at once, then the link)
    units = [(str(src), ["-O0"] + san)] + [(os.path.join(csrc, u), ["-O1"]) for u in ("bspnode_builder.cpp", "bsppaper_builder.cpp", "bvh_builder.cpp")]
    procs = [subprocess.Popen(common + flags + ["-c", u, "-o", str(tmp_path / ("u%d.o" % k))], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for k, (u, flags) in enumerate(units)]
    for pr in procs:
        out, _ = pr.communicate()
        assert pr.returncode == 0, out
    r = subprocess.run(["g++", "-pthread"] + san + [str(tmp_path / ("u%d.o" % k)) for k in range(len(units))] + ["-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
