// hprt device side — the light-centred shadow grid as the kernel sees it (host build and layout: ../shadow_grid.h) and the
// launcher of k_shadow_grid (shadow_grid.hip).
#pragma once
#include "kernels.h"

namespace hprt {

// The grid's device image (../shadow_grid.h, ShadowGridImage): blocks, 128 bytes per cell with the list's first two candidates in
// place, then — from byte recordsAt = 6 R^2 * 128 on — records, 48 bytes per further entry, the padding included; the first nNear
// records are the near list.  One allocation of imageBytes < 2^32, so that the kernel reads both through one buffer resource.
struct DevShadowGrid { const uint32_t *image; uint32_t imageBytes, recordsAt, nNear, R; };

// Any-hit results of rays that all end at the grid's light, d = fl(light - o): occ[slot] as LaunchTrace's any-hit form writes it.
// Persistent waves over the index queue (null: rays 0 .. n - 1), as the walks.
void LaunchShadowGrid(hipStream_t st, const DevScene &sc, const DevShadowGrid &g, const uint32_t *queue, const uint32_t *countPtr,
                      uint32_t countImm, uint32_t gridItems, const RayStream &rays, uint8_t *occ, uint32_t *workCounter);

}  // namespace hprt
