// hprt device side — the kd-aware general BSP walk (bsppaperkd_walk.hip): BSPKd::Intersect / IntersectP (accelerators/BSPKd.cpp:25-171).
#pragma once
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "bsppaper_walk.h"

namespace hprt {

// The attached kd-aware tree: the general BSP tree's device form (DevBspPaper: 8-byte node words, ordered primitive indices, one
// 16-byte axis entry per node) with BSPKdNode's flags (bsppaper_builder.h, BSPPAPERKD_*: the low 3 bits 0-2 a kd node's axis, 3 a
// leaf, 4 a plane node; aboveChild / nPrims << 3), and the kd counter pair, kdCounters[0] = kdTreeNodeTraversals, [1] =
// kdTreeNodeTraversalsP of the counting traces.  Only plane nodes' axis entries are ever read.
struct DevBspPaperKd {
    DevBspPaper t;
    unsigned long long *kdCounters;
};

// Drop-in for LaunchTrace on a scene with an attached bsppaperkd tree: same queue, ray and hit streams; DevCounters::nodesEntered[P]
// counts every interior node (kd and plane), and with `count` the kd ones go to kdCounters as well.  rayStats: interior nodes,
// leaves, primitive tests, kd interior nodes.
void LaunchBspPaperKdTrace(hipStream_t st, const DevScene &sc, const DevBspPaperKd &bp, bool anyHit, bool count, const uint32_t *queue,
                           const uint32_t *countPtr, uint32_t countImm, uint32_t gridItems, const RayStream &rays, const HitStream &hits,
                           uint8_t *occ, DevCounters *counters, uint32_t *workCounter, uint4 *rayStats);

}  // namespace hprt
