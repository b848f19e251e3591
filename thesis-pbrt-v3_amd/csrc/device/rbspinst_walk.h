// hprt device side — the two-level RBSP walks (rbspinst_walk.hip): RBSP::Intersect / IntersectP (accelerators/rbsp.cpp:405-547)
// or RBSPKd::Intersect / IntersectP (accelerators/rbspKd.cpp:490-638) on the top level and inside every object instance, joined
// by TransformedPrimitive::Intersect / IntersectP (core/primitive.cpp:77-102).
#pragma once
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "two_level.h"

namespace hprt {

// The attached trees in HBM.  nodes: the reference's 8-byte RBSPNode[] of the top-level tree (root 0) followed by every object
// tree's, with three changes: aboveChild and primitiveIndicesOffset of an object tree are rebased to the shared arrays, and the
// primitive word of a one-primitive leaf holds the ORDERED primitive index over all aggregates (DevScene numbering); primIdx is
// every tree's primitiveIndices mapped the same way.  Node order, leaf order and in-leaf order are the reference's.  Every tree is
// built over the same M directions: one table, one off, one mask.
struct DevRbspInst {
    const uint2 *nodes; uint32_t nNodes;
    const uint32_t *primIdx; uint32_t nPrimIdx;
    const DevInstEntry *entries; uint32_t nEntries;      // one per instance (DevScene::instances numbering)
    float lo[3], hi[3];                 // the top-level GenericBSP::bounds
    uint32_t depth;                     // top-level depth + deepest object depth + 1: the most todo entries a ray can hold
    uint32_t M, off, mask;              // directions; flags: leaf M | nPrims << off, interior axis | aboveChild << off
    float dirs[3 * 13];                 // getDirections(M) (accelerators/RBSPShared.h)
    unsigned long long *kdCounters;     // kd-aware trees: [0] kdTreeNodeTraversals, [1] kdTreeNodeTraversalsP of the counting traces
};

// Drop-in for LaunchTrace (kernels.h) on an instanced scene with attached two-level RBSP trees: same queue, ray and hit streams
// (hits.b carries the instance of the hit, as k_trace writes it), the RBSP walk's counters and per-ray statistics summed over both
// levels.  kdAware: the trees are rbspkd trees — axis nodes take the kd form and are counted apart (kdCounters, rayStats.w).
void LaunchRbspInstTrace(hipStream_t st, const DevScene &sc, const DevRbspInst &rb, bool kdAware, bool anyHit, bool count, const uint32_t *queue,
                         const uint32_t *countPtr, uint32_t countImm, uint32_t gridItems, const RayStream &rays, const HitStream &hits,
                         uint8_t *occ, DevCounters *counters, uint32_t *workCounter, uint4 *rayStats);

}  // namespace hprt
