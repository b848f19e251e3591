// hprt device side — the two-level general BSP walks (gfx950, wave64): BSP::Intersect / IntersectP (accelerators/BSP.cpp:27-165)
// or, kd-aware, BSPKd::Intersect / IntersectP (accelerators/BSPKd.cpp:25-171) over the top-level tree,
// TransformedPrimitive::Intersect / IntersectP (core/primitive.cpp:77-102) at every leaf primitive that is an object instance, and
// the same walk over the instance's own tree with the transformed ray — what an instanced Accelerator "bsppaper" / "bsppaperkd"
// scene is in the reference (pbrtObjectInstance, core/api.cpp:1794-1819).  The loop, the one todo list of both levels and the leaf
// loop are bspinst_walk (bspinst_walk.h); this file holds the two interior steps.
//
// Interior steps: those of bsppaper_walk.hip (BspPaperStep) and bsppaperkd_walk.hip (BspPaperKdStep), restated here operation for
// operation so that those units' code objects stay as they are.  They are pure functions of the node's axis and the ray they are
// given — the world ray on the top level, the instance's ray inside an instance: an object tree was built over the object's
// primitives in object space, so its split axes are object-space vectors and meet the transformed ray.  What the comments there say
// about +-inf, NaN and -0 components holds in instance space as it does in world space: the plain step takes full dot products
// against EVERY axis, the (1,0,0)-style axes of the axis sweep included; the kd-aware step takes the kd form at kd nodes and reads
// ray.d[axis], not invDir[axis], for the side.
//
// The axis fetch.  One 16-byte entry per node of the shared node array (DevBspPaperInst::axes).  Plain trees request it beside the
// node's 8-byte word (bspinst_walk's NODE_AXIS = 1, the form bsppaper_walk.hip ships), kd-aware trees only once the node word says
// "plane node" (NODE_AXIS = 3, the form bsppaperkd_walk.hip ships).  Both forms were chosen from single-level A/Bs (DESIGN.md §8d,
// §8e); for the two-level walk the choice is unmeasured (§8m).
//
// Built with -ffp-contract=off: every float operation is one IEEE rounding in the reference's order.
#include <hip/hip_runtime.h>
#include "bsppaperinst_walk.h"
#include "bspinst_walk.h"
#include "../bsppaper_builder.h"

#ifndef HPRT_BSPPAPERINST_LDS
#define HPRT_BSPPAPERINST_LDS 8
#endif
#define HPRT_BSPPAPERINST_BLOCK 256
// workgroups per CU (= waves per SIMD): as for the two-level RBSP walks, four for the triangle-only kernels (128 VGPRs: the
// two-level state plus the node's axis) and three with the quadric code (168), at which no variant spills a VGPR
#ifndef HPRT_BSPPAPERINST_WAVES
#define HPRT_BSPPAPERINST_WAVES 4
#endif
#define HPRT_BSPPAPERINST_QUAD_WAVES 3

namespace hprt {

static_assert(HPRT_BSPPAPERINST_LDS + HPRT_SPILL_STACK >= (int)BSPPAPER_TODO_MAX && HPRT_BSPPAPERINST_LDS + HPRT_SPILL_STACK >= (int)BSPPAPERKD_TODO_MAX,
              "LDS + deep-stack entries must hold the deepest pair of trees attach accepts");
static_assert(HPRT_DEEP_THREADS >= 256u * HPRT_BSPPAPERINST_BLOCK * HPRT_BSPPAPERINST_WAVES &&
                  HPRT_DEEP_THREADS >= 256u * HPRT_BSPPAPERINST_BLOCK * HPRT_BSPPAPERINST_QUAD_WAVES,
              "the deep-stack area must cover the two-level general BSP walks' grids");
static_assert(HPRT_BSPPAPERINST_LDS * HPRT_BSPPAPERINST_BLOCK * sizeof(uint2) == 16384, "8 todo entries x 256 threads x 8 bytes of LDS per workgroup");

// treeIntersectInterior with planeDistance (core/geometry.h:1837-1843): bsppaper_walk.hip's BspPaperStep
struct BspPaperInstStep {
    const float4 *axes;                 // HBM: one {x, y, z, 0} per node of the shared array
    __device__ __forceinline__ bool leaf(uint32_t flags) const { return (flags & BSPPAPER_MASK) != 0u; }
    __device__ __forceinline__ uint32_t high(uint32_t flags) const { return flags >> BSPPAPER_OFF; }
    __device__ __forceinline__ float4 axis(uint32_t node) const { return axes[node]; }
    __device__ __forceinline__ void plane(float4 a, uint32_t, float split, vec3 ro, vec3 rd, vec3, float *tPlane, bool *belowFirst) const {
        const float projectedO = a.x * ro.x + a.y * ro.y + a.z * ro.z;              // Dot(axis, ray.o)
        const float inverseProjectedD = 1 / (a.x * rd.x + a.y * rd.y + a.z * rd.z);  // 1 / Dot(axis, ray.d)
        *tPlane = (split - projectedO) * inverseProjectedD;
        *belowFirst = (projectedO < split) || (projectedO == split && inverseProjectedD <= 0);
    }
};

// BSPKdNode::intersectInterior (accelerators/BSPKd.h:59-83): bsppaperkd_walk.hip's BspPaperKdStep.  Both forms are evaluated and
// the operands selected (no divergent branch); o / invDir / d [axis] are picked by comparisons, never by a runtime index.
struct BspPaperKdInstStep {
    const float4 *axes;                 // HBM: one {x, y, z, 0} per node of the shared array, read for plane nodes only
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

// ANY_HIT: IntersectP; COUNT: counters and per-ray statistics (with KD, the kd share too); QUAD: the scene has spheres (the
// interval-arithmetic test is compiled in only then); KD: the trees are bsppaperkd trees.
template <bool ANY_HIT, bool COUNT, bool QUAD, bool KD>
__global__ __launch_bounds__(HPRT_BSPPAPERINST_BLOCK, QUAD ? HPRT_BSPPAPERINST_QUAD_WAVES : HPRT_BSPPAPERINST_WAVES) void k_bsppaperinstwalk(
    DevScene sc, DevBspPaperInst bp, const uint32_t *queue, const uint32_t *countPtr, uint32_t countImm, RayStream rays, HitStream hits, uint8_t *occ,
    DevCounters *counters, uint4 *rayStats, uint32_t *workCounter) {
    __shared__ uint2 stackMem[HPRT_BSPPAPERINST_LDS * HPRT_BSPPAPERINST_BLOCK];     // [entry][thread]: {node, tPlane} or {leaf node, position}
    if constexpr (KD) {
        BspPaperKdInstStep step{bp.axes, bp.kdCounters};
        bspinst_walk<ANY_HIT, COUNT, QUAD, HPRT_BSPPAPERINST_LDS, HPRT_BSPPAPERINST_BLOCK, BspPaperKdInstStep, true, 3>(
            sc, bp.nodes, bp.primIdx, (const float4 *)bp.entries, bp.lo, bp.hi, step, queue, countPtr, countImm, rays, hits, occ, counters, rayStats,
            workCounter, stackMem);
    } else {
        BspPaperInstStep step{bp.axes};
        bspinst_walk<ANY_HIT, COUNT, QUAD, HPRT_BSPPAPERINST_LDS, HPRT_BSPPAPERINST_BLOCK, BspPaperInstStep, false, 1>(
            sc, bp.nodes, bp.primIdx, (const float4 *)bp.entries, bp.lo, bp.hi, step, queue, countPtr, countImm, rays, hits, occ, counters, rayStats,
            workCounter, stackMem);
    }
}

void LaunchBspPaperInstTrace(hipStream_t st, const DevScene &sc, const DevBspPaperInst &bp, bool kdAware, bool anyHit, bool count, const uint32_t *queue,
                             const uint32_t *countPtr, uint32_t countImm, uint32_t gridItems, const RayStream &rays, const HitStream &hits,
                             uint8_t *occ, DevCounters *counters, uint32_t *workCounter, uint4 *rayStats) {
    LaunchTreeWalk<HPRT_BSPPAPERINST_BLOCK, HPRT_BSPPAPERINST_WAVES, HPRT_BSPPAPERINST_QUAD_WAVES>(st, sc, anyHit, count, gridItems, workCounter, [&](dim3 grid, dim3 block, auto a, auto c, auto q) {
        if (kdAware)
            hipLaunchKernelGGL((k_bsppaperinstwalk<decltype(a)::value, decltype(c)::value, decltype(q)::value, true>), grid, block, 0, st, sc, bp, queue, countPtr,
                               countImm, rays, hits, occ, counters, rayStats, workCounter);
        else
            hipLaunchKernelGGL((k_bsppaperinstwalk<decltype(a)::value, decltype(c)::value, decltype(q)::value, false>), grid, block, 0, st, sc, bp, queue, countPtr,
                               countImm, rays, hits, occ, counters, rayStats, workCounter);
    });
}

}  // namespace hprt
