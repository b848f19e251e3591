// hprt device side — what the two shadow-grid kernels share by name: k_shadow_grid (shadow_grid.hip, the point light's grid) and
// k_distant_grid (distant_grid.hip, the distant light's) run one lane machine, whose loop is grid_lanes_body.h, over the same
// device image (../shadow_grid.h, ShadowGridImage).  Here: the machine's states, the two tests on an entry's second word, and
// the sizing of a launch.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include "kernels.h"
#include "../shadow_grid.h"

namespace hprt {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// the ray's sixteenth lies in the part of the cell an entry's triangle reaches (../shadow_grid.h: the lower 16 bits of the entry's second word)
__device__ __forceinline__ bool sg_reaches(uint32_t w, uint32_t sub) {
    const uint32_t su = sub & 15u, sv = sub >> 4;
    return su >= (w & 15u) && su <= ((w >> 4) & 15u) && sv >= ((w >> 8) & 15u) && sv <= ((w >> 12) & 15u);
}

__device__ __forceinline__ float sg_key(uint32_t w) { return __uint_as_float(w & SG_KEY_MASK); }

// SG_BLOCK: the first four words of the cell's block wanted (its head, triangle 0, the key words of entries 1 and 2); SG_BLOCK2: the
// block's triangle 1; SG_OVER: the 48-byte record of entry i (the near list, a cell's list from its third entry on)
enum : int { SG_IDLE = 0, SG_RAY = 1, SG_BLOCK = 2, SG_BLOCK2 = 3, SG_OVER = 4, SG_BOX = 5 };

// Persistent waves: perCu workgroups per CU (what the kernel is compiled for), never more than the rays need; every wave takes its
// rays off the queue in chunks of 64 .. 512, about four per wave.  (HPRT_TRACE_MAX_BLOCKS and HPRT_TRACE_CHUNK_MAX: the walks' test
// hooks, a handful of waves working through many queue chunks each.)
struct GridLaunchSize { uint32_t blocks, chunk; };
inline GridLaunchSize grid_launch_size(uint32_t gridItems, uint32_t perCu) {
    static const uint32_t blockCap = [] { const char *e = getenv("HPRT_TRACE_MAX_BLOCKS"); return e ? (uint32_t)std::max(1, atoi(e)) : 0xffffffffu; }();
    static const uint32_t chunkMax = [] { const char *e = getenv("HPRT_TRACE_CHUNK_MAX"); return e ? (uint32_t)atoi(e) : 512u; }();
    const uint32_t blocks = std::min((uint32_t)(((size_t)gridItems + HPRT_TRACE_BLOCK - 1) / HPRT_TRACE_BLOCK), std::min(256u * perCu, blockCap));
    const uint32_t nWaves = blocks * (HPRT_TRACE_BLOCK / 64);
    const uint32_t chunk = gridItems / (nWaves * 4u);
    return {blocks, std::max(64u, std::min(chunkMax, chunk)) & ~63u};
}

}  // namespace hprt
