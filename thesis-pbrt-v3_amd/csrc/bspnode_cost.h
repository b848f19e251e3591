// hprt — the cost of one split candidate of a node-based BSP build (BuildBspNodeTree's costRange, bspnode_builder.cpp) over
// fixed-capacity storage, restated once as __host__ __device__ code over bsp_cost.h: its Cut, SurfaceArea, CompactNode,
// Capacities, Store and Work are used unchanged.  No allocation, every loop bounded by a capacity, every float operation one IEEE
// rounding in the vector code's order (both compilers build with -ffp-contract=off -fno-fast-math).
//
// A sweep's candidates share a handful of directions (nDirs per node, up to 2 nPrimitives candidates each), so what depends on
// the direction alone is computed once per direction (PrepareDir): DirectionId over the node's own list, the direction's place p
// in the compact table cdir[] and whether it enters the table.  A candidate is then 16 bytes (Cand: direction index, the sweep's
// counts, t) and costs the cut at t, the two areas, the empty bonus and the formula of its direction's kind:
//   kind 0   traversalCost + C                                                  (plain and withkd trees)
//   kind 1   kdTraversalCost + C                                                (a fastkd axis)
//   kind 2   BSP_ALPHA isectCost (N - 1) + kdTraversalCost + C, and costFixed = traversalCost + C   (a fastkd chosen direction)
// There is no extent test (the sweep emits only candidates strictly inside the k-DOP's extent) and no BVH.
// A candidate that would exceed a capacity sets *overflow, writes nothing past the storage and reports no cost.
#pragma once
#include "bsp_cost.h"

#define BSPNODE_MAX_SWEEP_DIRS 16     // the per-direction table; a node with more sweep directions is declined whole

namespace hprt {
namespace bspnodecost {

using bspcost::Edge;
using bspcost::Q;
using bspcost::Node;
using bspcost::Scalars;
using bspcost::Store;
using bspcost::Work;

enum : uint32_t { KIND_PLAIN = 0u, KIND_KD_AXIS = 1u, KIND_CHOSEN = 2u };

struct Cand { uint32_t k, nBelow, nAbove; float t; };                       // direction k of the sweep; the edge index stays on the host
struct SweepDir { float axis[3]; uint32_t kind; };                          // as the caller gives it
struct Dir { float axis[3]; uint32_t kind, id, p, entered, pad; };          // as every candidate of the direction reads it
static_assert(sizeof(Cand) == 16 && sizeof(SweepDir) == 16 && sizeof(Dir) == 32, "records shared with the device");

// What a sweep direction contributes to each of its candidates.  DirectionId: the first of the node's directions within half a
// degree, else a new one (id == M); p: the first compact direction not below id; entered: id owns no face of the mesh.
KDOP_HD Dir PrepareDir(const Node &nd, const SweepDir &sd) {
    Dir d;
    d.axis[0] = sd.axis[0]; d.axis[1] = sd.axis[1]; d.axis[2] = sd.axis[2]; d.kind = sd.kind; d.pad = 0;
    uint32_t id = nd.M;
    for (uint32_t i = 0; i < nd.M; ++i)
        if ((double)(nd.dirs[3 * i] * sd.axis[0] + nd.dirs[3 * i + 1] * sd.axis[1] + nd.dirs[3 * i + 2] * sd.axis[2]) > 0.999961923) { id = i; break; }
    uint32_t p = 0;
    while (p < nd.nD && nd.cdir[p] < id) ++p;
    d.id = id; d.p = p; d.entered = (p < nd.nD && nd.cdir[p] == id) ? 0u : 1u;
    return d;
}

// One candidate of costRange.  *cost / *costFixed: what costRange leaves in costs[k] / costsFixed[k] (the latter +inf unless the
// direction's kind is KIND_CHOSEN).  FASTKD false: every kind is KIND_PLAIN's formula.  Nothing is reported when *overflow is set.
template <bool FASTKD>
KDOP_HD void CostCandidate(const Node &nd, const Scalars &sc, const Dir &d, const Cand &c, const Store &st, float *cost, float *costFixed, uint8_t *overflow) {
    Work w;
    w.st = st; w.overflow = false;
    *cost = 0; *costFixed = bspcost::Inf(); *overflow = 1;
    if (nd.nE > st.capEdges || nd.M > BSP_MAX_DIRS || 2 * nd.nD > st.capFaces) return;
    const float axis[3] = {d.axis[0], d.axis[1], d.axis[2]};
    w.p = d.p; w.shift = d.entered ? 2u : 0u; w.id = d.id;
    const uint32_t nFaces = 2 * (nd.nD + (d.entered ? 1u : 0u));
    BSP_NOTE_MAX(1, nFaces);
    if (nFaces > st.capFaces) return;
    bspcost::Cut(w, nd.mesh, nd.nE, nFaces, c.t, axis);
    float areaBelow = 0, areaAbove = 0;
    if (!w.overflow) areaBelow = bspcost::SurfaceArea(w, false, nd, axis[0], axis[1], axis[2], nFaces);
    if (!w.overflow) areaAbove = bspcost::SurfaceArea(w, true, nd, axis[0], axis[1], axis[2], nFaces);
    if (w.overflow) return;
    *overflow = 0;
    const float pBelow = areaBelow * sc.invTotalSA;
    const float pAbove = areaAbove * sc.invTotalSA;
    const float eb = (c.nAbove == 0 || c.nBelow == 0) ? sc.emptyBonus : 0;
    const float BSP_ALPHA = 0.1f;
    if (!FASTKD || d.kind == KIND_PLAIN) {
        *cost = (float)sc.traversalCost + (float)sc.isectCost * (1 - eb) * (pBelow * (float)c.nBelow + pAbove * (float)c.nAbove);
    } else if (d.kind == KIND_KD_AXIS) {
        *cost = (float)sc.kdTraversalCost + (float)sc.isectCost * (1 - eb) * (pBelow * (float)c.nBelow + pAbove * (float)c.nAbove);
    } else {
        const float costIntersection = (float)sc.isectCost * (1 - eb) * (pBelow * (float)c.nBelow + pAbove * (float)c.nAbove);
        *costFixed = (float)sc.traversalCost + costIntersection;
        *cost = BSP_ALPHA * (float)sc.isectCost * (float)(sc.nPrimitives - 1) + (float)sc.kdTraversalCost + costIntersection;
    }
}

// Host: a whole node, one candidate after the other, over storage of the caller's (words: bspcost::kStoreWords 16-byte words or
// the exact need of the capacities in force, 4 capEdges + 2 capFaces; list: capFaceEdges bytes).  mesh / cdir / nD: CompactNode's.
// Every candidate's k is below nDirs <= BSPNODE_MAX_SWEEP_DIRS (the caller has checked).
inline void CostNode(const Edge *mesh, uint32_t nE, const float *dirs, uint32_t M, const uint32_t *cdir, uint32_t nD, bool fastKd, const Scalars &sc,
                     const SweepDir *sweep, uint32_t nDirs, const Cand *cands, size_t n, const uint32_t cap[4], Q *words, uint8_t *list, float *costs,
                     float *costsFixed, uint8_t *overflow) {
    Store st;
    st.left = words; st.right = words + 2 * (size_t)cap[0]; st.fv = words + 4 * (size_t)cap[0]; st.stride = 1;
    st.flist = list; st.fstride = 1; st.stack = nullptr; st.sstride = 1;
    st.capEdges = cap[0]; st.capFaces = cap[1]; st.capFaceEdges = cap[2]; st.capStack = 0;
    Node nd{};
    nd.mesh = mesh; nd.nE = nE; nd.dirs = dirs; nd.M = M; nd.cdir = cdir; nd.nD = nD;
    Dir table[BSPNODE_MAX_SWEEP_DIRS];
    for (uint32_t k = 0; k < nDirs; ++k) table[k] = PrepareDir(nd, sweep[k]);
    for (size_t k = 0; k < n; ++k) {
        float fixed;
        if (fastKd) CostCandidate<true>(nd, sc, table[cands[k].k], cands[k], st, &costs[k], &fixed, &overflow[k]);
        else CostCandidate<false>(nd, sc, table[cands[k].k], cands[k], st, &costs[k], &fixed, &overflow[k]);
        if (costsFixed) costsFixed[k] = fixed;
    }
}

}  // namespace bspnodecost
}  // namespace hprt
