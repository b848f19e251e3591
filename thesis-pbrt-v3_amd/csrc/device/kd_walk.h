// hprt device side — the kd-tree walk (kd_walk.hip): KdTreeAccel::Intersect / IntersectP (accelerators/kdtreeaccel.cpp:381-521).
#pragma once
#include <hip/hip_runtime.h>
#include "kernels.h"

namespace hprt {

// The attached tree in HBM.  nodes: the reference's 8-byte KdAccelNode[] (kdtree_builder.h) with one change: the primitive
// word of a one-primitive leaf holds the ORDERED primitive index (DevScene numbering), not the creation-order number; primIdx
// is primitiveIndices mapped the same way.  Node order, leaf order and in-leaf order are the reference's.
struct DevKd {
    const uint2 *nodes; uint32_t nNodes;
    const uint32_t *primIdx; uint32_t nPrimIdx;
    float lo[3], hi[3];                 // KdTreeAccel::bounds
    uint32_t depth;                     // interior levels of the deepest path: the most todo entries a ray can hold
};

// Drop-in for LaunchTrace (kernels.h) on a scene with an attached kd-tree: same queue, ray and hit streams, same counters
// (DevCounters: nodesFetched[P] = nbNodeTraversals[P], nodesEntered[P] = kdTreeNodeTraversals[P]) and per-ray statistics
// (rayStats: interior nodes, leaves, primitive tests).
void LaunchKdTrace(hipStream_t st, const DevScene &sc, const DevKd &kd, bool anyHit, bool count, const uint32_t *queue,
                   const uint32_t *countPtr, uint32_t countImm, uint32_t gridItems, const RayStream &rays, const HitStream &hits,
                   uint8_t *occ, DevCounters *counters, uint32_t *workCounter, uint4 *rayStats);

}  // namespace hprt
