// hprt device side — the two-level kd-tree walk (kdinst_walk.hip): KdTreeAccel::Intersect / IntersectP
// (accelerators/kdtreeaccel.cpp:381-521) on the top level and inside every object instance, joined by
// TransformedPrimitive::Intersect / IntersectP (core/primitive.cpp:77-102).
#pragma once
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "two_level.h"

namespace hprt {

// The attached trees in HBM.  nodes: the reference's 8-byte KdAccelNode[] of the top-level tree (root 0) followed by every object
// tree's, with three changes: aboveChild and primitiveIndicesOffset of an object tree are rebased to the shared arrays, and the
// primitive word of a one-primitive leaf holds the ORDERED primitive index over all aggregates (DevScene numbering); primIdx is
// every tree's primitiveIndices mapped the same way.  Node order, leaf order and in-leaf order are the reference's.
struct DevKdInst {
    const uint2 *nodes; uint32_t nNodes;
    const uint32_t *primIdx; uint32_t nPrimIdx;
    const DevInstEntry *entries; uint32_t nEntries;      // one per instance (DevScene::instances numbering)
    float lo[3], hi[3];                 // the top-level KdTreeAccel::bounds
    uint32_t depth;                     // top-level depth + deepest object depth + 1: the most todo entries a ray can hold
};

// Drop-in for LaunchTrace (kernels.h) on an instanced scene with attached two-level kd-trees: same queue, ray and hit streams
// (hits.b carries the instance of the hit, as k_trace writes it), the kd walk's counters and per-ray statistics summed over both
// levels.
void LaunchKdInstTrace(hipStream_t st, const DevScene &sc, const DevKdInst &kd, bool anyHit, bool count, const uint32_t *queue,
                       const uint32_t *countPtr, uint32_t countImm, uint32_t gridItems, const RayStream &rays, const HitStream &hits,
                       uint8_t *occ, DevCounters *counters, uint32_t *workCounter, uint4 *rayStats);

}  // namespace hprt
