// hprt device side — the two-level general BSP walks (bsppaperinst_walk.hip): BSP::Intersect / IntersectP
// (accelerators/BSP.cpp:27-165) or, kd-aware, BSPKd::Intersect / IntersectP (accelerators/BSPKd.cpp:25-171) on the top level and
// inside every object instance, joined by TransformedPrimitive::Intersect / IntersectP (core/primitive.cpp:77-102).
#pragma once
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "two_level.h"

namespace hprt {

// The attached trees in HBM: DevKdInst's shared fields (kdinst_walk.h) over the first 8 bytes of the reference's 20-byte BSPNode[]
// / BSPKdNode[] — the top-level tree (root 0) followed by every object tree's, aboveChild and primitiveIndicesOffset rebased, the
// primitive word of a one-primitive leaf and primIdx holding ORDERED primitive indices over all aggregates.  axes: every node's
// splitAxis as {x, y, z, 0}, one 16-byte entry per node of `nodes` in the same order (zero for leaves, for the kd nodes of a
// kd-aware tree and for the one-primitive leaf that stands for a tree-less object), so exactly nNodes entries: an object's node
// finds its OBJECT-SPACE axis at its own index.
struct DevBspPaperInst {
    const uint2 *nodes; uint32_t nNodes;
    const uint32_t *primIdx; uint32_t nPrimIdx;
    const DevInstEntry *entries; uint32_t nEntries;      // one per instance (DevScene::instances numbering)
    float lo[3], hi[3];                 // the top-level GenericBSP::bounds
    uint32_t depth;                     // top-level depth + deepest object depth + 1: the most todo entries a ray can hold
    const float4 *axes;
    unsigned long long *kdCounters;     // kd-aware trees: [0] kdTreeNodeTraversals, [1] kdTreeNodeTraversalsP of the counting traces
};

// Drop-in for LaunchTrace (kernels.h) on an instanced scene with attached two-level general BSP trees: same queue, ray and hit
// streams (hits.b carries the instance of the hit, as k_trace writes it), the general BSP walk's counters and per-ray statistics
// summed over both levels.  kdAware: the trees are bsppaperkd trees — kd nodes take the kd form and are counted apart (kdCounters,
// rayStats.w).
void LaunchBspPaperInstTrace(hipStream_t st, const DevScene &sc, const DevBspPaperInst &bp, bool kdAware, bool anyHit, bool count, const uint32_t *queue,
                             const uint32_t *countPtr, uint32_t countImm, uint32_t gridItems, const RayStream &rays, const HitStream &hits,
                             uint8_t *occ, DevCounters *counters, uint32_t *workCounter, uint4 *rayStats);

}  // namespace hprt
