// hprt device side — the general BSP walk (bsppaper_walk.hip): BSP::Intersect / IntersectP (accelerators/BSP.cpp:27-165).
#pragma once
#include <hip/hip_runtime.h>
#include "kernels.h"

namespace hprt {

// The attached tree in HBM.  nodes: the first 8 bytes of the reference's 20-byte BSPNode[] (bsppaper_builder.h: flags leaf
// 1 | nPrims << 1, interior aboveChild << 1) with the primitive word of a one-primitive leaf holding the ORDERED primitive index;
// primIdx is primitiveIndices mapped the same way.  axes: the node's splitAxis as {x, y, z, 0}, one 16-byte entry per node
// (zero for leaves).  Node order, leaf order and in-leaf order are the reference's.
struct DevBspPaper {
    const uint2 *nodes; uint32_t nNodes;
    const uint32_t *primIdx; uint32_t nPrimIdx;
    float lo[3], hi[3];                 // GenericBSP::bounds
    uint32_t depth;                     // interior levels of the deepest path: the most todo entries a ray can hold
    const float4 *axes;
};

// Drop-in for LaunchTrace (kernels.h) on a scene with an attached bsppaper tree: same queue, ray and hit streams, same counters
// (DevCounters: nodesFetched[P] = nbNodeTraversals[P], nodesEntered[P] = bspTreeNodeTraversals[P]) and per-ray statistics
// (rayStats: interior nodes, leaves, primitive tests).
void LaunchBspPaperTrace(hipStream_t st, const DevScene &sc, const DevBspPaper &bp, bool anyHit, bool count, const uint32_t *queue,
                         const uint32_t *countPtr, uint32_t countImm, uint32_t gridItems, const RayStream &rays, const HitStream &hits,
                         uint8_t *occ, DevCounters *counters, uint32_t *workCounter, uint4 *rayStats);

}  // namespace hprt
