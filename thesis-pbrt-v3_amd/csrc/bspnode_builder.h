// hprt — the fork's node-based BSP trees, whose K split directions are chosen anew at every node: Accelerator "bsparbitrary",
// "bspcluster", "bsprandom" (BSPNodeBased::buildTree, accelerators/bspNodeBased.cpp:27-223), their "...withkd" forms
// (bspNodeBasedWithKd.cpp: the three axes in front of K - 3 chosen directions) and their "...fastkd" forms
// (BSPNodeBasedFastKd::buildTree, bspNodeBasedFastKd.cpp:28-330: kd-aware costs over BSPKdNode).  The plain and withkd trees are
// BSP trees over BSPNode — structurally bsppaper trees (BspPaperTree, kdAware false); the fastkd trees are BSPKd trees over
// BSPKdNode — structurally bsppaperkd trees (kdAware true).  Both go to the walks that exist (device/bsppaper_walk.hip,
// device/bsppaperkd_walk.hip).
//
// The one deliberate departure from the reference: it seeds std::mt19937 from std::random_device, so no two of its builds agree;
// here the engine is seeded with BspNodeParams::seed (default: std::mt19937's own default seed, 5489), so that a scene file
// renders the same tree every time.  Everything drawn from the engine is drawn as the reference draws it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>
#include "bspnode_cost.h"
#include "bsppaper_builder.h"

namespace hprt {

enum : int { BSPNODE_ARBITRARY = 0, BSPNODE_CLUSTER = 1, BSPNODE_RANDOM = 2 };      // chooseArbitraryNormals, calculateClusterMeans, chooseRandomDirections
enum : int { BSPNODE_PLAIN = 0, BSPNODE_WITHKD = 1, BSPNODE_FASTKD = 2 };
enum : uint32_t { BSPNODE_DEFAULT_SEED = 5489u };                                    // std::mt19937::default_seed

// One node's candidates, as costFn sees them (bspnode_cost.h).  mesh / dirs: the node's k-DOP and its own direction list
// (cur.dirs); sweep: the directions the node sweeps (nodeDirs), each with the kind of its cost formula; cands: every candidate in
// the scan's (direction, edge) order, k indexing sweep.  nDirs is not always K: arbitrary yields min(np, K) directions, cluster np
// of them when np <= K, fastkd with K = 3 none besides the axes; two may be equal, and one may be (0, 0, 0) (it has no candidate).
struct BspNodeCostRequest {
    const kdopcost::Edge *mesh; uint32_t nEdges;          // face ids below 2 M
    const float *dirs; uint32_t M;
    const bspnodecost::SweepDir *sweep; uint32_t nDirs;
    bool fastKd;
    bspcost::Scalars sc;
    const bspnodecost::Cand *cands; size_t n;
    float *costs, *costsFixed;                            // costsFixed: NULL unless fastKd; +inf except for KIND_CHOSEN
    uint8_t *overflow;                                    // 1: not costed (a capacity of the costing was exceeded)
    uint32_t level;                                       // the node's depth below the root (diagnostics)
};

// costFn, costMinCandidates, stats, costDone: the costing hook (cost_hook.h; the device-assisted build, hprt_bspnode_build_device).
// The chooser has drawn before costFn is called and costFn draws nothing, so the tree of a seed is the same either way.
struct BspNodeParams : CostHook<BspNodeCostRequest> {
    int chooser = BSPNODE_CLUSTER, form = BSPNODE_PLAIN;
    int nDirections = 3;                  // "nbDirections": K; the withkd / fastkd forms choose K - 3 and need K >= 3
    uint32_t seed = BSPNODE_DEFAULT_SEED; // "seed"
    int isectCost = 80, travCost = 5;     // "intersectcost", "traversalcost"
    int kdTravCost = 1;                   // "kdtraversalcost" (fastkd)
    float emptyBonus = 0.f;               // "emptybonus"
    int maxPrims = 1, maxDepth = -1;      // "maxprims", "maxdepth" (-1: round(2 + 1.6 Log2Int(N)))
    int threads = 0;                      // candidate evaluation threads: 0 = OMP_NUM_THREADS (else 16), at most 16
};

// "bsparbitrary" ... "bsprandomfastkd" -> chooser and form; false for any other name
bool BspNodeAccelerator(const std::string &name, int *chooser, int *form);

// Why BuildBspNodeTree refuses these parameters whatever the primitives are (an unknown chooser or form, a K the reference's build
// is undefined for), or an empty string.  The device-assisted entries ask before they open a device, so that such a build is
// refused with the host entry's message on every machine.
std::string BspNodeRefuseParams(const BspNodeParams &p);

// n primitives in creation order, as BuildBspPaperTree takes them.  Returns an empty string, or why the tree cannot be built: where
// the reference's build is undefined (K < 3 for withkd / fastkd, a drawn index equal to the primitive count, the fastkd case in
// which only the second minimum is set) and where it would write past its primitive buffer.
std::string BuildBspNodeTree(size_t n, const float *bmin, const float *bmax, const float *tri9, const uint8_t *isTri, const BspNodeParams &p,
                             BspPaperTree *out);

// The candidates of rq costed with the builder's own code (CutMeasure over the vector meshes and costRange's formulas) on the
// calling thread: what the diagnostics hook hprt_debug_bspnode_cost calls impl 0.  overflow is cleared.
void BspNodeCostVector(const BspNodeCostRequest &rq);

// The direction choosers on their own (diagnostics; tests/test_bspnode_host.py): `draws` calls of the chooser over the triangles p9
// (all n of them are the node's primitives, in order) from one engine seeded with `seed`.  Per call, counts gets the number of
// directions returned and dirs their components; returns an error string as BuildBspNodeTree does.
std::string BspNodeChoose(int chooser, uint32_t K, uint32_t seed, size_t n, const float *tri9, uint32_t draws, std::vector<uint32_t> *counts,
                          std::vector<float> *dirs);

}  // namespace hprt
