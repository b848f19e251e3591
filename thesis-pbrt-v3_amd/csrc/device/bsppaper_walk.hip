// hprt device side — the general BSP walk (gfx950, wave64): BSP::Intersect / IntersectP (accelerators/BSP.cpp:27-165) with the leaf
// loops of treeIntersectLeaf / treeIntersectPLeaf (BSP.h:74-120), restated operation for operation, over the reference's node
// array (bsppaper_walk.h, DevBspPaper).  The loop, the todo list and the leaf loop are bsp_walk (bsp_walk.h); this file holds
// the interior step.  It serves every tree over BSPNode: bsppaper, and the node-based bsparbitrary, bspcluster and bsprandom.
//
// Interior step (treeIntersectInterior with planeDistance, core/geometry.h:1837-1843): pO = Dot(axis, o), iD = 1 / Dot(axis, d)
// as full float dot products against the node's OWN axis — also for the (1,0,0)-style axes of the axis sweep, for the reasons
// rbsp_walk.hip gives.  The axis is the one per-node datum the 8-byte node does not hold: a 16-byte entry per node in HBM
// (DevBspPaper::axes), requested by bsp_walk together with the node's 8-byte word (NODE_AXIS = 1) so that the two latencies
// overlap; a leaf visit fetches 16 bytes it does not use.  HPRT_BSPPAPER_LATE_AXIS=1 requests it only after the leaf test
// instead (NODE_AXIS = 2: a dependent round trip per interior node) — the A/B of DESIGN.md §8d.
//
// Built with -ffp-contract=off: every float operation is one IEEE rounding in the reference's order.
#include <hip/hip_runtime.h>
#include "bsppaper_walk.h"
#include "bsp_walk.h"
#include "../bsppaper_builder.h"

#ifndef HPRT_BSPPAPER_LDS
#define HPRT_BSPPAPER_LDS 8
#endif
#define HPRT_BSPPAPER_BLOCK 256
// workgroups per CU (= waves per SIMD): as for the kd and RBSP walks, six for the triangle-only kernels, four with the quadric code
#ifndef HPRT_BSPPAPER_WAVES
#define HPRT_BSPPAPER_WAVES 6
#endif
#define HPRT_BSPPAPER_QUAD_WAVES 4
#ifndef HPRT_BSPPAPER_LATE_AXIS
#define HPRT_BSPPAPER_LATE_AXIS 0
#endif

namespace hprt {

static_assert(HPRT_BSPPAPER_LDS + HPRT_SPILL_STACK >= (int)BSPPAPER_TODO_MAX, "LDS + deep-stack entries must hold the deepest tree attach accepts");
static_assert(HPRT_DEEP_THREADS >= 256u * HPRT_BSPPAPER_BLOCK * HPRT_BSPPAPER_WAVES, "the deep-stack area must cover the walk's grid");

struct BspPaperStep {
    const float4 *axes;                 // HBM: one {x, y, z, 0} per node
    __device__ __forceinline__ bool leaf(uint32_t flags) const { return (flags & 1u) != 0u; }
    __device__ __forceinline__ uint32_t high(uint32_t flags) const { return flags >> 1; }
    __device__ __forceinline__ float4 axis(uint32_t node) const { return axes[node]; }
    __device__ __forceinline__ void plane(float4 a, uint32_t, float split, vec3 ro, vec3 rd, vec3, float *tPlane, bool *belowFirst) const {
        const float projectedO = a.x * ro.x + a.y * ro.y + a.z * ro.z;              // Dot(axis, ray.o)
        const float inverseProjectedD = 1 / (a.x * rd.x + a.y * rd.y + a.z * rd.z);  // 1 / Dot(axis, ray.d)
        *tPlane = (split - projectedO) * inverseProjectedD;
        *belowFirst = (projectedO < split) || (projectedO == split && inverseProjectedD <= 0);
    }
};

// ANY_HIT: IntersectP; COUNT: counters and per-ray statistics; QUAD: the scene has spheres (the interval-arithmetic test is
// compiled in only then).
template <bool ANY_HIT, bool COUNT, bool QUAD>
__global__ __launch_bounds__(HPRT_BSPPAPER_BLOCK, QUAD ? HPRT_BSPPAPER_QUAD_WAVES : HPRT_BSPPAPER_WAVES) void k_bsppaperwalk(
    DevScene sc, DevBspPaper bp, const uint32_t *queue, const uint32_t *countPtr, uint32_t countImm, RayStream rays, HitStream hits, uint8_t *occ,
    DevCounters *counters, uint4 *rayStats, uint32_t *workCounter) {
    __shared__ uint2 stackMem[HPRT_BSPPAPER_LDS * HPRT_BSPPAPER_BLOCK];     // [entry][thread]: {node, tPlane}
    BspPaperStep step{bp.axes};
    bsp_walk<ANY_HIT, COUNT, QUAD, HPRT_BSPPAPER_LDS, HPRT_BSPPAPER_BLOCK, BspPaperStep, false, HPRT_BSPPAPER_LATE_AXIS ? 2 : 1>(
        sc, bp.nodes, bp.primIdx, bp.lo, bp.hi, step, queue, countPtr, countImm, rays, hits, occ, counters, rayStats, workCounter, stackMem);
}

void LaunchBspPaperTrace(hipStream_t st, const DevScene &sc, const DevBspPaper &bp, bool anyHit, bool count, const uint32_t *queue,
                         const uint32_t *countPtr, uint32_t countImm, uint32_t gridItems, const RayStream &rays, const HitStream &hits,
                         uint8_t *occ, DevCounters *counters, uint32_t *workCounter, uint4 *rayStats) {
    LaunchTreeWalk<HPRT_BSPPAPER_BLOCK, HPRT_BSPPAPER_WAVES, HPRT_BSPPAPER_QUAD_WAVES>(st, sc, anyHit, count, gridItems, workCounter, [&](dim3 grid, dim3 block, auto a, auto c, auto q) {
        hipLaunchKernelGGL((k_bsppaperwalk<decltype(a)::value, decltype(c)::value, decltype(q)::value>), grid, block, 0, st, sc, bp, queue, countPtr,
                           countImm, rays, hits, occ, counters, rayStats, workCounter);
    });
}

}  // namespace hprt
