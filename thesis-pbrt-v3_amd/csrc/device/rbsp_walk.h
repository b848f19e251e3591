// hprt device side — the RBSP walk (rbsp_walk.hip): RBSP::Intersect / IntersectP (accelerators/rbsp.cpp:405-547).
#pragma once
#include <hip/hip_runtime.h>
#include "kernels.h"

namespace hprt {

// The attached tree in HBM.  nodes: the reference's 8-byte RBSPNode[] (rbsp_builder.h) with one change: the primitive word of a
// one-primitive leaf holds the ORDERED primitive index (DevScene numbering), not the creation-order number; primIdx is
// primitiveIndices mapped the same way.  Node order, leaf order and in-leaf order are the reference's.
struct DevRbsp {
    const uint2 *nodes; uint32_t nNodes;
    const uint32_t *primIdx; uint32_t nPrimIdx;
    float lo[3], hi[3];                 // GenericBSP::bounds
    uint32_t depth;                     // interior levels of the deepest path: the most todo entries a ray can hold
    uint32_t M, off, mask;              // directions; flags: leaf M | nPrims << off, interior axis | aboveChild << off
    float dirs[3 * 13];                 // getDirections(M) (accelerators/RBSPShared.h)
};

// Drop-in for LaunchTrace (kernels.h) on a scene with an attached RBSP tree: same queue, ray and hit streams, same counters
// (DevCounters: nodesFetched[P] = nbNodeTraversals[P], nodesEntered[P] = bspTreeNodeTraversals[P]) and per-ray statistics
// (rayStats: interior nodes, leaves, primitive tests).
void LaunchRbspTrace(hipStream_t st, const DevScene &sc, const DevRbsp &rb, bool anyHit, bool count, const uint32_t *queue,
                     const uint32_t *countPtr, uint32_t countImm, uint32_t gridItems, const RayStream &rays, const HitStream &hits,
                     uint8_t *occ, DevCounters *counters, uint32_t *workCounter, uint4 *rayStats);

}  // namespace hprt
