// hprt device side — the light-aligned shadow grid of a distant light as the kernel sees it (host build and layout:
// ../distant_grid.h) and the launcher of k_distant_grid (distant_grid.hip, lib/libhprt_dg.so).
#pragma once
#include "kernels.h"
#include "../distant_grid.h"

namespace hprt {

// The grid's device image, laid out as DevShadowGrid's (shadow_grid.h; ../shadow_grid.h, ShadowGridImage) with R^2 cells: blocks, 128
// bytes per cell, then — from byte recordsAt = R^2 * 128 on — records, 48 bytes each, the padding included; the first nNear records
// are the near list.  One allocation of imageBytes < 2^32.  f: what a ray's cell and key limit are computed from.
struct DevDistantGrid { const uint32_t *image; uint32_t imageBytes, recordsAt, nNear, R; DgFrame f; };

// Any-hit results of rays that all run towards the grid's light, d = fl(fl(p + w * 2 worldRadius) - o): occ[slot] as LaunchTrace's
// any-hit form writes it.  Persistent waves over the index queue (null: rays 0 .. n - 1), as the walks.
void LaunchDistantGrid(hipStream_t st, const DevScene &sc, const DevDistantGrid &g, const uint32_t *queue, const uint32_t *countPtr,
                       uint32_t countImm, uint32_t gridItems, const RayStream &rays, uint8_t *occ, uint32_t *workCounter);

}  // namespace hprt
