"""bsp_cost.h on the host: the fixed-capacity restatement of one general BSP split candidate (extent test, DirectionId, cut, the two
surface areas over the child's directions, NodeBvh::count, the cost formulas) against the builder's vector code, bit for bit, on
the candidates of real build nodes (handed out by the builder itself); the flags at the compiled and at lowered capacities; the
validation of the diagnostics hook; the device entries without a device; a stand-alone sanitizer run of the header.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bsp_cost_nodes as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ids(k):
    kind = k[0] if isinstance(k[0], str) else "%s%d" % (k[0][1], k[0][0])
    return kind + ("-kd" if k[1] else "")


def _agree(hprt, nd, impl, **caps):
    """costs nd with impl; asserts that every unflagged candidate carries impl 0's cost, fixed cost and counts; returns the flags"""
    rc0, c0, f0, n0, o0 = B.cost(hprt, nd, 0)
    rc, c, f, n, o = B.cost(hprt, nd, impl, **caps)
    assert rc0 == 0 and rc == 0 and not o0.any() and set(np.unique(o)) <= {0, 1}
    ok = o == 0
    assert B.equal_where(ok, c, c0) and B.equal_where(ok, f, f0) and B.equal_where(ok, n, n0)
    return o


@pytest.mark.parametrize("key", B.node_sets(), ids=_ids)
def test_restatement_equals_the_vector_code(hprt, key):
    """impl 1 == impl 0 == the costs, fixed costs and counts the builder's own costRange gave, on every candidate of the first 64
    nodes; no flag is set at the compiled capacities, so nothing here (or in the GPU tests) passes by falling back"""
    nodes = B.nodes_of(key)
    assert len(nodes) == B.NODES
    total = planes = 0
    for nd in nodes:
        bc, bf, bn = B.builder_results(nd)
        rc0, c0, f0, n0, o0 = B.cost(hprt, nd, 0)
        rc1, c1, f1, n1, o1 = B.cost(hprt, nd, 1)
        assert rc0 == 0 and rc1 == 0 and not o0.any() and not o1.any()
        assert B.same_bits(c0, bc) and B.same_bits(f0, bf) and np.array_equal(n0, bn)
        assert B.same_bits(c1, c0) and B.same_bits(f1, f0) and np.array_equal(n1, n0)
        assert int(nd["n_axis"]) == int((nd["cands"]["k"] < 3).sum())
        total += len(c0); planes += len(c0) - int(nd["n_axis"])
    assert total > 1000 and planes > 500


def _deep_nodes(hprt, kd):
    nodes = B.build_nodes(hprt, kd, p9=dict(B.soups(300))["grid1"], max_nodes=400)
    return [nd for nd in nodes if nd["level"] >= 8 and len(nd["dirs"]) > 9]


@pytest.mark.parametrize("kd", (False, True), ids=("plain", "kd"))
def test_a_deep_node_with_a_grown_direction_list(hprt, kd):
    """nodes at least 8 levels below the root whose direction list has grown past the three axes: the compaction of the faces and
    a candidate's direction entering the table in the middle or at the end"""
    deep = _deep_nodes(hprt, kd)
    assert deep, "no node of the build is 8 levels deep with more than three directions"
    most = max(len(nd["dirs"]) // 3 for nd in deep)
    assert most > 3
    for nd in deep[:48]:
        assert nd["level"] >= 8 and len(nd["dirs"]) // 3 > 3
        assert not _agree(hprt, nd, 1).any()


def faceless_direction_nodes(nodes, limit=12):
    """nodes whose direction list carries, in its middle, a direction that owns no face of the mesh and lies within half a degree
    of some plane candidates' axes without being equal to them: those candidates take ITS id, its faces enter the compact table
    between the others, and their areas are measured along ITS vector, not along the candidates' axes (killeroo-simple's build
    meets this; the small builds do not, so it is made here).  The face ids of the directions behind it move up by two."""
    out = []
    for nd in nodes:
        c = nd["cands"]
        pl = np.nonzero(c["k"] == B.PLANE)[0]
        dirs = nd["dirs"].reshape(-1, 3)
        if len(pl) == 0 or len(dirs) < 4:
            continue
        axis = c["axis"][pl[len(pl) // 2]].astype(np.float64)
        if (dirs.astype(np.float64) @ axis).max() > 0.9999:      # one of the node's directions already takes this candidate
            continue
        tilt = axis + 0.004 * np.roll(axis, 1)                    # about a quarter of a degree off
        tilt = (tilt / np.linalg.norm(tilt)).astype(np.float32)
        assert float(tilt.astype(np.float64) @ axis) > 0.99997 and not np.array_equal(tilt, c["axis"][pl[len(pl) // 2]])
        edges = nd["edges"].copy()
        for f in ("f1", "f2"):
            edges[f] = np.where(edges[f] >= 6, edges[f] + 2, edges[f])
        new = dict(nd, edges=edges, dirs=np.concatenate([dirs[:3], tilt[None], dirs[3:]]).astype(np.float32).ravel())
        out.append(new)
        if len(out) == limit:
            break
    return out


def test_a_direction_that_owns_no_face_keeps_its_own_vector(hprt):
    nodes = faceless_direction_nodes(_deep_nodes(hprt, False) + _deep_nodes(hprt, True))
    assert len(nodes) >= 4
    moved = 0
    for nd in nodes:
        rc0, c0, f0, n0, o0 = B.cost(hprt, nd, 0)
        assert rc0 == 0
        assert not _agree(hprt, nd, 1).any()
        # the inserted direction did take some candidates: their costs differ from the costs along their own axes
        plain = B.cost(hprt, dict(nd, dirs=np.concatenate([nd["dirs"][:9], np.float32([0, 0, -1]), nd["dirs"][12:]])), 0)
        moved += int((plain[1].view(np.uint32) != c0.view(np.uint32)).sum())
    assert moved > 0


LOWERED = (("maxEdges", 16), ("maxFaces", 10), ("maxFaceEdges", 5), ("maxStack", 4))


@pytest.mark.parametrize("field,value", LOWERED, ids=[f for f, _ in LOWERED])
def test_lowered_capacity_flags_and_never_lies(hprt, field, value):
    """each capacity lowered until some candidates are flagged; an unflagged one carries the vector code's cost and counts"""
    flagged = clean = 0
    for key in (((200, "grid1"), False), ((300, "random"), True)):
        for nd in B.nodes_of(key):
            o = _agree(hprt, nd, 1, **{field: value})
            if field == "maxEdges" and len(nd["edges"]) > value:
                assert o.all()      # a node's mesh beyond the capacity is declined whole
            if field == "maxStack":
                assert not o[: int(nd["n_axis"])].any()      # axis candidates walk no BVH
            flagged += int(o.sum()); clean += int((o == 0).sum())
    assert flagged > 0 and clean > 0


def test_out_of_extent_planes_cost_inf_and_keep_their_counts(hprt):
    seen = 0
    for key in B.node_sets():
        for nd in B.nodes_of(key)[1:]:
            cands = nd["cands"].copy()
            pl = cands["k"] == B.PLANE
            cands["nBelow"][pl] = 77; cands["nAbove"][pl] = 99
            for impl in (0, 1):
                rc, c, f, n, o = B.cost(hprt, nd, impl, cands=cands, zero_counts=False)
                assert rc == 0 and not o.any()
                out = pl & np.isposinf(c)
                assert np.isposinf(f[out]).all() and (n[out, 0] == 77).all() and (n[out, 1] == 99).all()
            seen += int(out.sum())
    assert seen > 100


def test_debug_hook_rejects_malformed_input(hprt):
    nd = next(n for n in B.nodes_of(((300, "random"), False)) if n["n_axis"] < len(n["cands"]))
    E = hprt.E_INVALID
    for impl in (0, 1):
        assert B.cost(hprt, nd, impl)[0] == 0
        assert B.cost(hprt, nd, impl, M=0)[0] == E
        bad = nd["edges"].copy(); bad["f1"][3] = 2 * (len(nd["dirs"]) // 3)
        assert B.cost(hprt, nd, impl, edges=bad)[0] == E
        bad = nd["edges"].copy(); bad["f2"][0] = 0xffffffff
        assert B.cost(hprt, nd, impl, edges=bad)[0] == E
        bad = nd["cands"].copy(); bad["k"][0] = 7                        # neither an axis nor a plane
        assert B.cost(hprt, nd, impl, cands=bad)[0] == E
        bad = nd["cands"].copy(); bad["k"][-1] = 1                       # an axis candidate among the planes
        assert B.cost(hprt, nd, impl, cands=bad)[0] == E
        assert B.cost(hprt, nd, impl, n_axis=len(nd["cands"]) + 1)[0] == E
        assert B.cost(hprt, nd, impl, bvh=nd["bvh"][:0])[0] == E          # planes without a BVH
        bad = nd["bvh"].copy(); bad["offset"][0] = len(bad) + 5           # second child outside the array
        assert B.cost(hprt, nd, impl, bvh=bad)[0] == E
        bad = nd["prim_order"].copy(); bad[0] = len(bad)
        assert B.cost(hprt, nd, impl, prim_order=bad)[0] == E
        bad = nd["prim_nums"].copy(); bad[-1] = 0x7fffffff
        assert B.cost(hprt, nd, impl, prim_nums=bad)[0] == E
        for f in B.CAPS:
            assert B.cost(hprt, nd, impl, **{f: 4096})[0] == E            # may only lower the capacity
    assert B.cost(hprt, nd, 3)[0] == E and B.cost(hprt, nd, -1)[0] == E
    assert hprt.lib.hprt_debug_bsp_cost(None, 0, 1, None, None, None, None) == E
    # a mesh of more edges than the capacity: valid input, the node is declined whole, nothing costed
    big = np.concatenate([nd["edges"]] * 12)
    assert len(big) > 64
    rc, c, f, n, o = B.cost(hprt, nd, 1, edges=big)
    assert rc == 0 and o.all()


def test_device_entries_without_a_device(hprt):
    """hprt_bsppaper*_build*_device: HPRT_E_NO_DEVICE and *out NULL where there is no HIP device; the host refusals come first"""
    import torch
    p9 = dict(B.soups(200))["random"]
    vp = p9.ctypes.data_as(C.c_void_p)
    prm = hprt.BspPaperParams(80, 5, 0.0, 1, -1, 0)
    kprm = hprt.BspPaperKdParams(80, 5, 1, 0.0, 1, -1, 0)
    for name, q in (("hprt_bsppaper_build_from_triangles_device", prm), ("hprt_bsppaperkd_build_from_triangles_device", kprm)):
        h = C.c_void_p(0xdead)
        st = hprt.BuildDeviceStats()
        rc = getattr(hprt.lib, name)(p9.shape[0], vp, C.byref(q), None, C.byref(st), C.byref(h))
        if torch.cuda.is_available():
            assert rc == 0 and h.value
            getattr(hprt.lib, name.split("_build")[0] + "_destroy")(h)
        else:
            assert rc == hprt.E_NO_DEVICE and h.value is None
    m = hprt.Model.load(B.DODECA)
    if not torch.cuda.is_available():
        for cls in (hprt.BspPaper, hprt.BspPaperKd):
            with pytest.raises(hprt.HprtError) as e:
                cls(m, isect_cost=80, device=0)
            assert e.value.code == hprt.E_NO_DEVICE
            with pytest.raises(hprt.HprtError) as e:
                cls.from_triangles(p9, device=0, min_candidates=1)
            assert e.value.code == hprt.E_NO_DEVICE
    inst = hprt.Model.load(os.path.join(os.path.dirname(B.DODECA), "simple_instanced.hprt"))
    for name in ("hprt_bsppaper_build_device", "hprt_bsppaperkd_build_device"):
        h = C.c_void_p(0xdead)
        assert getattr(hprt.lib, name)(inst._h, None, None, None, C.byref(h)) == hprt.E_UNSUPPORTED and h.value is None
    assert hprt.BspPaper(m, isect_cost=80).build_stats is None       # the host build keeps no device statistics


SANITIZER_DRIVER = r"""
// bsp_cost.h on a handful of real nodes, at the compiled and at lowered capacities, against the builder's vector code; built with
// -fsanitize=address,undefined and run on its own
#include <cstdio>
#include <cstring>
#include <vector>
#include "bsppaper_builder.h"
#include "bvh_builder.h"
using namespace hprt;
using namespace hprt::bspcost;
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
    isTri[7] = 0; isTri[23] = 0;                       // two primitives that project their bound's corners
    int fails = 0; size_t nodes = 0, flagged = 0, costed = 0;
    for (int kd = 0; kd < 2; ++kd) {
        BspPaperParams p; p.kdAware = kd != 0; p.threads = 1; p.costMinCandidates = 1;
        p.costFn = [&](const BspCostRequest &rq, std::string *) -> int {
            if (nodes >= 40) return 1;
            ++nodes;
            std::vector<float> c0(rq.n), f0(rq.n);
            std::vector<uint8_t> o0(rq.n);
            std::vector<Cand> cs(rq.cands, rq.cands + rq.n);
            BspCostRequest v = rq; v.cands = cs.data(); v.costs = c0.data(); v.costsFixed = f0.data(); v.overflow = o0.data();
            BspCostVector(v);
            const uint32_t lowered[3][4] = {{0, 0, 0, 0}, {16, 10, 5, 3}, {24, 8, 6, 2}};
            for (const auto &low : lowered) {
                Scalars sc = rq.sc; sc.maxEdges = low[0]; sc.maxFaces = low[1]; sc.maxFaceEdges = low[2]; sc.maxStack = low[3];
                uint32_t cap[4];
                if (!Capacities(sc, cap)) { ++fails; continue; }
                if (rq.nEdges > cap[0] || rq.M > BSP_MAX_DIRS) continue;
                std::vector<Edge> mesh(rq.nEdges); std::vector<uint32_t> cdir(rq.M); uint32_t nD = 0;
                CompactNode(rq.mesh, rq.nEdges, rq.M, mesh.data(), cdir.data(), &nD);
                if (2 * nD > cap[1]) continue;
                // exactly the capacity's storage, so that a write past it is a heap overflow the sanitizer sees
                std::vector<Q> left(2 * cap[0]), right(2 * cap[0]), fv(2 * cap[1]);
                std::vector<uint8_t> list(cap[2]); std::vector<uint32_t> stack(cap[3]);
                const Store st{left.data(), right.data(), fv.data(), 1, list.data(), 1, stack.data(), 1, cap[0], cap[1], cap[2], cap[3]};
                const Node nd{mesh.data(), rq.nEdges, rq.dirs, rq.M, cdir.data(), nD, rq.bvh, rq.nBvh, rq.primOrder, rq.primNums, rq.nPrims,
                              rq.bmin, rq.bmax, rq.tri9, rq.isTri, (uint32_t)rq.nTotal};
                for (size_t k = 0; k < rq.n; ++k) {
                    float c, f; uint32_t nb, na; uint8_t o;
                    Cand in = rq.cands[k];
                    if (in.k == 33u) { in.nBelow = 0; in.nAbove = 0; }
                    CostCandidate(nd, rq.kdAware, sc, in, st, &c, &f, &nb, &na, &o);
                    ++costed;
                    if (o) { ++flagged; if (!low[0]) ++fails; continue; }
                    const bool outside = in.k == 33u && c0[k] == Inf();
                    if (std::memcmp(&c, &c0[k], 4) || std::memcmp(&f, &f0[k], 4)) ++fails;
                    if (!outside && (nb != cs[k].nBelow || na != cs[k].nAbove)) ++fails;
                    if (outside && (nb != 0 || na != 0)) ++fails;
                }
            }
            return 1;      // the build itself goes on with its own code
        };
        BspPaperTree t;
        const std::string err = BuildBspPaperTree(n, lo.data(), hi.data(), p9.data(), isTri.data(), p, &t);
        if (!err.empty()) { std::printf("build: %s\n", err.c_str()); ++fails; }
    }
    std::printf("nodes %zu candidates %zu flagged %zu fails %d\n", nodes, costed, flagged, fails);
    return (fails == 0 && nodes >= 40 && flagged > 0 && costed > flagged) ? 0 : 1;
}
"""


def test_header_runs_clean_under_the_sanitizers(tmp_path):
    """a stand-alone program with its own main over bsp_cost.h, built with -fsanitize=address,undefined and run directly: the
    storage is sized to the capacity in force, so a write past it would be reported"""
    src = tmp_path / "bsp_cost_san.cpp"
    src.write_text(SANITIZER_DRIVER)
    csrc = os.path.join(ROOT, "thesis-pbrt-v3_amd", "csrc")
    exe = str(tmp_path / "bsp_cost_san")
    common = ["g++", "-std=c++17", "-Wall", "-Werror", "-pthread", "-ffp-contract=off", "-fno-fast-math", "-I" + csrc]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # the driver, and with it every instantiation of the header it drives, is built under the sanitizers; the builder that hands
    # out the nodes is the library's own source, built plainly beside it (three compilers at once, then the link)
    units = [(str(src), ["-O0"] + san), (os.path.join(csrc, "bsppaper_builder.cpp"), ["-O1"]), (os.path.join(csrc, "bvh_builder.cpp"), ["-O1"])]
    procs = [subprocess.Popen(common + flags + ["-c", u, "-o", str(tmp_path / ("u%d.o" % k))], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for k, (u, flags) in enumerate(units)]
    for pr in procs:
        out, _ = pr.communicate()
        assert pr.returncode == 0, out
    r = subprocess.run(["g++", "-pthread"] + san + [str(tmp_path / ("u%d.o" % k)) for k in range(3)] + ["-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
