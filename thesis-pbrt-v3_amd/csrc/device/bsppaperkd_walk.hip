// hprt device side — the kd-aware general BSP walk (gfx950, wave64): BSPKd::Intersect / IntersectP (accelerators/BSPKd.cpp:25-171)
// with BSPKdNode::intersectInterior (BSPKd.h:59-83) and its leaf loops (:85-124), restated operation for operation over the
// reference's node array (bsppaperkd_walk.h, DevBspPaperKd).  The loop, the todo list and the leaf loop are bsp_walk (bsp_walk.h)
// with its kd share counted; this file holds the interior step.
//
// Interior step.  kd nodes (flags & 7 < 3) take the kd form, planeDistance(split, ray, invDir, axis):
//   tPlane = (split - o[axis]) * invDir[axis],  belowFirst = o[axis] < split || (o[axis] == split && d[axis] <= 0);
// plane nodes (flags & 7 == 4) the general BSP walk's full dot products against the node's own axis (bsppaper_walk.hip).  The two
// forms differ where a component is +-inf, NaN or -0 and where d[axis] = +-0 meets an origin on the split, so
// they are not merged: both are evaluated and the operands selected by comparisons on the flags, never by a runtime index, so no
// per-ray array lands in scratch.
//
// The axis fetch.  Only plane nodes have an axis, and most visits are to kd nodes and leaves, so the 16-byte entry is requested
// only once the node word says "plane node" (bsp_walk's NODE_AXIS = 3: a dependent round trip, on those nodes alone).
// HPRT_BSPPAPERKD_EAGER_AXIS=1 requests it beside every node's 8-byte word instead, as the bsppaper walk does (NODE_AXIS = 1:
// no dependent trip, 16 unused bytes at every kd node and leaf) — the A/B of DESIGN.md §8e.
//
// Built with -ffp-contract=off: every float operation is one IEEE rounding in the reference's order.
#include <hip/hip_runtime.h>
#include "bsppaperkd_walk.h"
#include "bsp_walk.h"
#include "../bsppaper_builder.h"

#ifndef HPRT_BSPPAPERKD_LDS
#define HPRT_BSPPAPERKD_LDS 8
#endif
#define HPRT_BSPPAPERKD_BLOCK 256
// workgroups per CU (= waves per SIMD): as for the other tree walks, six for the triangle-only kernels (512 / 6 = 85 -> at most 80
// VGPRs), four with the quadric code (128 VGPRs)
#ifndef HPRT_BSPPAPERKD_WAVES
#define HPRT_BSPPAPERKD_WAVES 6
#endif
#define HPRT_BSPPAPERKD_QUAD_WAVES 4
#ifndef HPRT_BSPPAPERKD_EAGER_AXIS
#define HPRT_BSPPAPERKD_EAGER_AXIS 0
#endif

namespace hprt {

static_assert(HPRT_BSPPAPERKD_LDS + HPRT_SPILL_STACK >= (int)BSPPAPERKD_TODO_MAX, "LDS + deep-stack entries must hold the deepest tree attach accepts");
static_assert(HPRT_DEEP_THREADS >= 256u * HPRT_BSPPAPERKD_BLOCK * HPRT_BSPPAPERKD_WAVES, "the deep-stack area must cover the walk's grid");
static_assert(HPRT_BSPPAPERKD_LDS * HPRT_BSPPAPERKD_BLOCK * sizeof(uint2) == 16384, "8 todo entries x 256 threads x 8 bytes of LDS per workgroup");

struct BspPaperKdStep {
    const float4 *axes;                 // HBM: one {x, y, z, 0} per node, read for plane nodes only
    unsigned long long *kdCounters;     // [0] kdTreeNodeTraversals, [1] kdTreeNodeTraversalsP
    __device__ __forceinline__ bool leaf(uint32_t flags) const { return (flags & BSPPAPERKD_MASK) == BSPPAPERKD_LEAF; }
    __device__ __forceinline__ uint32_t high(uint32_t flags) const { return flags >> BSPPAPERKD_OFF; }
    __device__ __forceinline__ bool kd(uint32_t flags) const { return (flags & BSPPAPERKD_MASK) < 3u; }
    __device__ __forceinline__ bool has_axis(uint32_t flags) const { return (flags & BSPPAPERKD_MASK) > BSPPAPERKD_LEAF; }
    __device__ __forceinline__ float4 axis(uint32_t node) const { return axes[node]; }
    __device__ __forceinline__ void plane(float4 a, uint32_t flags, float split, vec3 ro, vec3 rd, vec3 invDir, float *tPlane, bool *belowFirst) const {
        const uint32_t axis = flags & BSPPAPERKD_MASK;
        const float projectedO = a.x * ro.x + a.y * ro.y + a.z * ro.z;              // Dot(axis, ray.o)
        const float inverseProjectedD = 1 / (a.x * rd.x + a.y * rd.y + a.z * rd.z);  // 1 / Dot(axis, ray.d)
        const float oA = axis == 0u ? ro.x : (axis == 1u ? ro.y : ro.z);             // ray.o[axis]
        const float iA = axis == 0u ? invDir.x : (axis == 1u ? invDir.y : invDir.z);
        const float dA = axis == 0u ? rd.x : (axis == 1u ? rd.y : rd.z);            // ray.d[axis]
        const bool kdNode = axis < 3u;
        const float o = kdNode ? oA : projectedO, inv = kdNode ? iA : inverseProjectedD, side = kdNode ? dA : inverseProjectedD;
        *tPlane = (split - o) * inv;
        *belowFirst = (o < split) || (o == split && side <= 0);
    }
    // one atomic per wave: the wave's kd interior nodes
    __device__ __forceinline__ void kd_count_add(bool anyHit, uint32_t n) const {
        for (int s = 32; s > 0; s >>= 1) n += __shfl_down(n, s);
        if (__lane_id() == 0) atomicAdd(&kdCounters[anyHit ? 1 : 0], (unsigned long long)n);
    }
};

// ANY_HIT: IntersectP; COUNT: counters and per-ray statistics (with the kd share); QUAD: the scene has spheres.
template <bool ANY_HIT, bool COUNT, bool QUAD>
__global__ __launch_bounds__(HPRT_BSPPAPERKD_BLOCK, QUAD ? HPRT_BSPPAPERKD_QUAD_WAVES : HPRT_BSPPAPERKD_WAVES) void k_bsppaperkdwalk(
    DevScene sc, DevBspPaperKd bp, const uint32_t *queue, const uint32_t *countPtr, uint32_t countImm, RayStream rays, HitStream hits, uint8_t *occ,
    DevCounters *counters, uint4 *rayStats, uint32_t *workCounter) {
    __shared__ uint2 stackMem[HPRT_BSPPAPERKD_LDS * HPRT_BSPPAPERKD_BLOCK];     // [entry][thread]: {node, tPlane}
    BspPaperKdStep step{bp.t.axes, bp.kdCounters};
    bsp_walk<ANY_HIT, COUNT, QUAD, HPRT_BSPPAPERKD_LDS, HPRT_BSPPAPERKD_BLOCK, BspPaperKdStep, true, HPRT_BSPPAPERKD_EAGER_AXIS ? 1 : 3>(
        sc, bp.t.nodes, bp.t.primIdx, bp.t.lo, bp.t.hi, step, queue, countPtr, countImm, rays, hits, occ, counters, rayStats, workCounter, stackMem);
}

void LaunchBspPaperKdTrace(hipStream_t st, const DevScene &sc, const DevBspPaperKd &bp, bool anyHit, bool count, const uint32_t *queue,
                           const uint32_t *countPtr, uint32_t countImm, uint32_t gridItems, const RayStream &rays, const HitStream &hits,
                           uint8_t *occ, DevCounters *counters, uint32_t *workCounter, uint4 *rayStats) {
    LaunchTreeWalk<HPRT_BSPPAPERKD_BLOCK, HPRT_BSPPAPERKD_WAVES, HPRT_BSPPAPERKD_QUAD_WAVES>(st, sc, anyHit, count, gridItems, workCounter, [&](dim3 grid, dim3 block, auto a, auto c, auto q) {
        hipLaunchKernelGGL((k_bsppaperkdwalk<decltype(a)::value, decltype(c)::value, decltype(q)::value>), grid, block, 0, st, sc, bp, queue, countPtr,
                           countImm, rays, hits, occ, counters, rayStats, workCounter);
    });
}

}  // namespace hprt
