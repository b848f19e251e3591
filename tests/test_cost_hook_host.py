"""The builders' costing hook (csrc/cost_hook.h) without a GPU, through BuildRbspTree: a costFn that declines every node, one that
costs with kdop_cost.h and flags every third candidate, and two that fail.  The device builds reach these paths only on a GPU; the
diagnostics sinks reach only the flag-everything path.  A stand-alone driver built from the library's own source."""
import os
import subprocess

import pytest

from conftest import ROOT

DRIVER = r"""
#include <algorithm>
#include <cstdio>
#include <type_traits>
#include <utility>
#include <cstring>
#include <string>
#include <vector>
#include "rbsp_builder.h"
using namespace hprt;
static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("%s line %d: %s\n", mode, __LINE__, #c); ++fails; } } while (0)

static const size_t N = 200;
static const uint32_t M = 7, MIN_CANDS = 64;
static std::vector<float> lo, hi, tri9;
static std::vector<uint8_t> isTri;

static uint32_t lcg = 20240607u;
static float Rand() { lcg = lcg * 1664525u + 1013904223u; return (float)(lcg >> 8) * (1.f / 16777216.f); }
static void Scene() {
    tri9.resize(9 * N); lo.resize(3 * N); hi.resize(3 * N); isTri.assign(N, 1);
    for (size_t i = 0; i < N; ++i) {
        float c[3] = {Rand(), Rand(), Rand()};
        for (int v = 0; v < 3; ++v)
            for (int d = 0; d < 3; ++d) tri9[9 * i + 3 * v + d] = c[d] + 0.2f * (Rand() - 0.5f);
        for (int d = 0; d < 3; ++d) {
            float a = tri9[9 * i + d], b = tri9[9 * i + 3 + d], e = tri9[9 * i + 6 + d];
            lo[3 * i + d] = std::min(std::min(a, b), e); hi[3 * i + d] = std::max(std::max(a, b), e);
        }
    }
}
static bool SameTree(const RbspTree &a, const RbspTree &b) {
    return a.nodes.size() == b.nodes.size() && a.primIndices.size() == b.primIndices.size() &&
           std::memcmp(a.nodes.data(), b.nodes.data(), a.nodes.size() * sizeof(RbspNode)) == 0 &&
           (a.primIndices.empty() || std::memcmp(a.primIndices.data(), b.primIndices.data(), a.primIndices.size() * 4) == 0);
}
// The nodes a build costs, read off its tree: every interior node, and every leaf of more than maxPrims (1) primitives above the
// depth limit (it reached the scan and found no split worth taking)
static uint64_t CostedNodes(const RbspTree &t) {
    const uint32_t off = RbspBitOffset(M), mask = RbspBitMask(M);
    uint64_t costed = 0;
    std::vector<std::pair<uint32_t, uint32_t>> todo{{0u, 0u}};      // node, level
    while (!todo.empty()) {
        const uint32_t k = todo.back().first, level = todo.back().second;
        todo.pop_back();
        const RbspNode &nd = t.nodes[k];
        if ((nd.b & mask) == M) { if ((nd.b >> off) > 1 && level < t.maxDepth) ++costed; continue; }
        ++costed;
        todo.push_back({k + 1, level + 1}); todo.push_back({nd.b >> off, level + 1});
    }
    return costed;
}
// kdop_cost.h over one request; every third candidate flagged uncosted, and whatever exceeds the fixed-capacity storage
static uint64_t CostRestated(const RbspCostRequest &rq) {
    using namespace kdopcost;
    std::vector<Q> words(kStoreWords);
    uint8_t list[KDOP_MAX_FACE_EDGES];
    Store st;
    st.left = words.data(); st.right = words.data() + 2 * KDOP_MAX_EDGES; st.fv = words.data() + 4 * KDOP_MAX_EDGES; st.stride = 1;
    st.flist = list; st.fstride = 1; st.cap = KDOP_MAX_EDGES;
    uint64_t flagged = 0;
    for (size_t k = 0; k < rq.n; ++k) {
        float cost = 0, fixed = 0;
        uint8_t ovf = 1;
        if (rq.nEdges <= KDOP_MAX_EDGES) CostCandidate(rq.mesh, rq.nEdges, rq.dirs, rq.M, rq.kdAware, rq.sc, rq.cands[k], st, &cost, &fixed, &ovf);
        if (k % 3 == 2) ovf = 1;
        rq.costs[k] = ovf ? -1.f : cost;                             // a flagged candidate's cost is rubbish the repair must replace
        if (rq.costsFixed) rq.costsFixed[k] = ovf ? -1.f : fixed;
        rq.overflow[k] = ovf;
        flagged += ovf;
    }
    return flagged;
}

static void Run(bool kdAware) {
    const char *mode = kdAware ? "kd-aware" : "plain";
    RbspParams base;
    base.nDirections = (int)M; base.kdAware = kdAware; base.threads = 2;
    RbspTree plain;
    std::string err = BuildRbspTree(N, lo.data(), hi.data(), tri9.data(), isTri.data(), base, &plain);
    EXPECT(err.empty());
    EXPECT(plain.nodes.size() > 100);
    using Stats = std::remove_pointer<decltype(base.stats)>::type;

    {   // (a) a hook that declines every node
        RbspParams p = base;
        Stats bs;
        uint64_t calls = 0, done = 0;
        p.costMinCandidates = MIN_CANDS; p.stats = &bs;
        p.costFn = [&](const RbspCostRequest &rq, std::string *) -> int { ++calls; EXPECT(rq.n >= MIN_CANDS); return 1; };
        p.costDone = [&](const RbspCostRequest &) { ++done; };
        RbspTree t;
        err = BuildRbspTree(N, lo.data(), hi.data(), tri9.data(), isTri.data(), p, &t);
        EXPECT(err.empty());
        EXPECT(SameTree(t, plain));
        EXPECT(calls > 0 && done == 0);
        EXPECT(bs.nodesDevice == 0 && bs.candidatesDevice == 0 && bs.candidatesRecosted == 0 && bs.secondsDevice == 0);
        EXPECT(bs.nodesHost == CostedNodes(plain));
        EXPECT(bs.nodesHost > calls);                                // (nodes below the threshold count too)
    }
    {   // (b) kdop_cost.h, every third candidate flagged
        RbspParams p = base;
        Stats bs;
        uint64_t calls = 0, done = 0, handed = 0, flagged = 0;
        p.costMinCandidates = MIN_CANDS; p.stats = &bs;
        p.costFn = [&](const RbspCostRequest &rq, std::string *) -> int {
            ++calls; handed += rq.n;
            EXPECT(rq.n >= MIN_CANDS);
            EXPECT(done + 1 == calls);                               // costDone has run for every node before this one
            for (size_t k = 0; k < rq.n; ++k) EXPECT(rq.overflow[k] == 0);
            flagged += CostRestated(rq);
            return 0;
        };
        p.costDone = [&](const RbspCostRequest &rq) {
            ++done;
            EXPECT(done == calls);
            // after the repair: every cost is the host's own (RbspCostVector is costRange over a caller's mesh)
            std::vector<float> costs(rq.n), fixed(rq.n);
            std::vector<uint8_t> ovf(rq.n);
            RbspCostRequest host = rq;
            host.costs = costs.data(); host.costsFixed = rq.costsFixed ? fixed.data() : nullptr; host.overflow = ovf.data();
            RbspCostVector(host);
            size_t bad = 0;
            for (size_t k = 0; k < rq.n; ++k) {
                bad += std::memcmp(&costs[k], &rq.costs[k], 4) != 0;
                if (rq.costsFixed && rq.cands[k].d >= 3) bad += std::memcmp(&fixed[k], &rq.costsFixed[k], 4) != 0;      // (only oblique ones are read)
            }
            EXPECT(bad == 0);
            EXPECT((rq.costsFixed != nullptr) == rq.kdAware);
        };
        RbspTree t;
        err = BuildRbspTree(N, lo.data(), hi.data(), tri9.data(), isTri.data(), p, &t);
        EXPECT(err.empty());
        EXPECT(SameTree(t, plain));
        EXPECT(calls > 1 && done == calls);
        EXPECT(bs.nodesDevice == calls);
        EXPECT(flagged >= handed / 3 - calls && flagged < handed);   // (some candidates were costed by the hook, some were not)
        EXPECT(bs.candidatesRecosted == flagged);
        EXPECT(bs.candidatesDevice + bs.candidatesRecosted == handed);
        EXPECT(bs.nodesDevice + bs.nodesHost == CostedNodes(plain));
        EXPECT(bs.secondsDevice > 0);
    }
    {   // (c) a failure with a message, on the second call
        RbspParams p = base;
        int calls = 0;
        p.costMinCandidates = MIN_CANDS;
        p.costFn = [&](const RbspCostRequest &rq, std::string *e) -> int {
            if (++calls == 2) { *e = "the second node went wrong"; return -1; }
            CostRestated(rq);
            return 0;
        };
        RbspTree t;
        err = BuildRbspTree(N, lo.data(), hi.data(), tri9.data(), isTri.data(), p, &t);
        EXPECT(err == "the second node went wrong");
        EXPECT(calls == 2);
    }
    {   // (d) a failure without one
        RbspParams p = base;
        int calls = 0;
        p.costMinCandidates = MIN_CANDS;
        p.costFn = [&](const RbspCostRequest &, std::string *) -> int { ++calls; return -1; };
        RbspTree t;
        err = BuildRbspTree(N, lo.data(), hi.data(), tri9.data(), isTri.data(), p, &t);
        EXPECT(err == "the costing hook failed");
        EXPECT(calls == 1);
    }
}
int main() {
    Scene();
    Run(false);
    Run(true);
    return fails ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("cost_hook")
    src = d / "hook.cpp"
    src.write_text(DRIVER)
    csrc = os.path.join(ROOT, "thesis-pbrt-v3_amd", "csrc")
    exe = str(d / "hook")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror", "-pthread", "-I" + csrc, str(src),
                        os.path.join(csrc, "rbsp_builder.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_hook_declines_flags_and_fails(driver):
    """200 seeded random triangles, M = 7, plain and kd-aware, costMinCandidates 64.  (a) costFn returns 1: the hook-less tree byte
    for byte, nothing on the device, nodesHost every node the build costed (read off the tree).  (b) costFn costs with
    kdopcost::CostCandidate and flags every third candidate: the same tree, candidatesRecosted the number flagged, device + recosted
    the candidates handed over, never fewer than 64 candidates a call, costDone once per costed node after the repair with the
    host's own costs.  (c) -1 with a message on the second call: BuildRbspTree returns it.  (d) -1 without one: "the costing hook
    failed"."""
    r = subprocess.run([driver], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
