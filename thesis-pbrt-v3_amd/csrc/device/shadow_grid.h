// hprt device side — the light-centred shadow grid as the kernel sees it (host build and layout: ../shadow_grid.h) and the
// launcher of k_shadow_grid (shadow_grid.hip).
#pragma once
#include "kernels.h"

namespace hprt {

// cellStart[6 R^2 + 1], entries[nEntries] of {ordered primitive | SG_SINGLE, depth key}; entries[0 .. nNear) is the near list
struct DevShadowGrid { const uint32_t *cellStart; const uint2 *entries; uint32_t nEntries, nNear, R; };

// Any-hit results of rays that all end at the grid's light, d = fl(light - o): occ[slot] as LaunchTrace's any-hit form writes it.
// Persistent waves over the index queue (null: rays 0 .. n - 1), as the walks.
void LaunchShadowGrid(hipStream_t st, const DevScene &sc, const DevShadowGrid &g, const uint32_t *queue, const uint32_t *countPtr,
                      uint32_t countImm, uint32_t gridItems, const RayStream &rays, uint8_t *occ, uint32_t *workCounter);

}  // namespace hprt
