// hprt device side — the rbspkd walk (rbspkd_walk.hip): RBSPKd::Intersect / IntersectP (accelerators/rbspKd.cpp:490-638).
#pragma once
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "rbsp_walk.h"

namespace hprt {

// The attached kd-aware tree: the RBSP tree's device form (DevRbsp: the same node layout, ordered primitive indices and direction
// table) and the kd counter pair, kdCounters[0] = kdTreeNodeTraversals, [1] = kdTreeNodeTraversalsP of the counting traces.
struct DevRbspKd {
    DevRbsp t;
    unsigned long long *kdCounters;
};

// Drop-in for LaunchTrace on a scene with an attached rbspkd tree: same queue, ray and hit streams; DevCounters::nodesEntered[P]
// counts every interior node (kd and oblique), and with `count` the kd ones go to kdCounters as well.  rayStats: interior nodes,
// leaves, primitive tests, kd interior nodes.
void LaunchRbspKdTrace(hipStream_t st, const DevScene &sc, const DevRbspKd &rb, bool anyHit, bool count, const uint32_t *queue,
                       const uint32_t *countPtr, uint32_t countImm, uint32_t gridItems, const RayStream &rays, const HitStream &hits,
                       uint8_t *occ, DevCounters *counters, uint32_t *workCounter, uint4 *rayStats);
// LaunchPixelStats for the kd share: rayStats.w of the traced rays added to pixKd[anyHit][nPix] (the same pixel mapping)
void LaunchPixelKdStats(hipStream_t st, const uint4 *rayStats, const float4 *ids, const uint32_t *queue, const uint32_t *countPtr,
                        uint32_t countImm, uint32_t gridItems, uint32_t nPix, bool anyHit, uint32_t *pixKd);
// local pixel -> film pixel for the kd share: out2[plane * filmPixels + filmIndex], plane 0 closest hit, 1 any hit
void LaunchPixelKdStatsToFilm(hipStream_t st, const uint32_t *pixKd, const uint32_t *pixelXY, uint32_t nPix, int cx0, int cy0, int width,
                              size_t filmPixels, unsigned long long *out2);

}  // namespace hprt
