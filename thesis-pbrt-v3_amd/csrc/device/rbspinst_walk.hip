// hprt device side — the two-level RBSP walks (gfx950, wave64): RBSP::Intersect / IntersectP (accelerators/rbsp.cpp:405-547) or,
// kd-aware, RBSPKd::Intersect / IntersectP (accelerators/rbspKd.cpp:490-638) over the top-level tree,
// TransformedPrimitive::Intersect / IntersectP (core/primitive.cpp:77-102) at every leaf primitive that is an object instance, and
// the same walk over the instance's own tree with the transformed ray — what an instanced Accelerator "rbsp" / "rbspkd" scene is
// in the reference (pbrtObjectInstance, core/api.cpp:1794-1819).  The loop, the one todo list of both levels and the leaf loop are
// bspinst_walk (bspinst_walk.h); this file holds the two interior steps.
//
// Interior steps: those of rbsp_walk.hip (RbspStep) and rbspkd_walk.hip (RbspKdStep), restated here operation for operation so
// that those units' code objects stay as they are.  They are pure functions of the ray they are given — the world ray on the top
// level, the instance's ray inside an instance — and what the comments there say about +-inf, NaN and -0 components holds in
// instance space as it does in world space: the plain step takes full dot products for EVERY direction, the axis directions
// included (rbsp-3 does not borrow the kd walk's component shortcut), the kd-aware step takes the kd form at axis nodes and reads
// ray.d[axis], not invDir[axis], for the side.  The direction table depends on M only, so all trees share the one table in LDS
// (3 * 13 floats per workgroup).
//
// Built with -ffp-contract=off: every float operation is one IEEE rounding in the reference's order.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "rbspinst_walk.h"
#include "bspinst_walk.h"
#include "../rbsp_builder.h"

#ifndef HPRT_RBSPINST_LDS
#define HPRT_RBSPINST_LDS 8
#endif
#define HPRT_RBSPINST_BLOCK 256
// workgroups per CU (= waves per SIMD): as for the two-level kd walk, four for the triangle-only kernels — the two-level state
// (the instance's ray next to the positions of both levels) needs more than the 80 registers six waves leave — and three with the
// quadric code, whose interval-arithmetic call would otherwise push some of that state into scratch
#ifndef HPRT_RBSPINST_WAVES
#define HPRT_RBSPINST_WAVES 4
#endif
#define HPRT_RBSPINST_QUAD_WAVES 3

namespace hprt {

static_assert(HPRT_RBSPINST_LDS + HPRT_SPILL_STACK >= (int)RBSP_TODO_MAX, "LDS + deep-stack entries must hold the deepest pair of trees attach accepts");
static_assert(HPRT_DEEP_THREADS >= 256u * HPRT_RBSPINST_BLOCK * HPRT_RBSPINST_WAVES && HPRT_DEEP_THREADS >= 256u * HPRT_RBSPINST_BLOCK * HPRT_RBSPINST_QUAD_WAVES,
              "the deep-stack area must cover the two-level RBSP walks' grids");

// RBSPNode::intersectInterior with planeDistance (core/geometry.h:1837-1843): rbsp_walk.hip's RbspStep
struct RbspInstStep {
    const float *dirs;                  // LDS: 3 * M floats
    uint32_t M, off, mask;
    __device__ __forceinline__ bool leaf(uint32_t flags) const { return (flags & mask) == M; }
    __device__ __forceinline__ uint32_t high(uint32_t flags) const { return flags >> off; }
    __device__ __forceinline__ void plane(uint32_t flags, float split, vec3 ro, vec3 rd, vec3, float *tPlane, bool *belowFirst) const {
        const float *d = dirs + 3 * (flags & mask);
        const float dx = d[0], dy = d[1], dz = d[2];
        const float projectedO = dx * ro.x + dy * ro.y + dz * ro.z;              // Dot(direction, ray.o)
        const float inverseProjectedD = 1 / (dx * rd.x + dy * rd.y + dz * rd.z);  // 1 / Dot(direction, ray.d)
        *tPlane = (split - projectedO) * inverseProjectedD;
        *belowFirst = (projectedO < split) || (projectedO == split && inverseProjectedD <= 0);
    }
};

// RBSPKdNode::intersectInterior (accelerators/rbspKd.cpp:69-92): rbspkd_walk.hip's RbspKdStep.  Both forms are evaluated and the
// operands selected (no divergent branch); o / invDir / d [axis] are picked by comparisons, never by a runtime index.
struct RbspKdInstStep {
    const float *dirs;                  // LDS: 3 * M floats
    uint32_t M, off, mask;
    unsigned long long *kdCounters;     // [0] kdTreeNodeTraversals, [1] kdTreeNodeTraversalsP
    __device__ __forceinline__ bool leaf(uint32_t flags) const { return (flags & mask) == M; }
    __device__ __forceinline__ uint32_t high(uint32_t flags) const { return flags >> off; }
    __device__ __forceinline__ bool kd(uint32_t flags) const { return (flags & mask) < 3u; }
    __device__ __forceinline__ void plane(uint32_t flags, float split, vec3 ro, vec3 rd, vec3 invDir, float *tPlane, bool *belowFirst) const {
        const uint32_t axis = flags & mask;
        const float *d = dirs + 3 * axis;
        const float dx = d[0], dy = d[1], dz = d[2];
        const float projectedO = dx * ro.x + dy * ro.y + dz * ro.z;              // Dot(direction, ray.o)
        const float inverseProjectedD = 1 / (dx * rd.x + dy * rd.y + dz * rd.z);  // 1 / Dot(direction, ray.d)
        const float oA = axis == 0u ? ro.x : (axis == 1u ? ro.y : ro.z);          // ray.o[axis]
        const float iA = axis == 0u ? invDir.x : (axis == 1u ? invDir.y : invDir.z);
        const float dA = axis == 0u ? rd.x : (axis == 1u ? rd.y : rd.z);         // ray.d[axis]
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
// interval-arithmetic test is compiled in only then); KD: the trees are rbspkd trees.
template <bool ANY_HIT, bool COUNT, bool QUAD, bool KD>
__global__ __launch_bounds__(HPRT_RBSPINST_BLOCK, QUAD ? HPRT_RBSPINST_QUAD_WAVES : HPRT_RBSPINST_WAVES) void k_rbspinstwalk(DevScene sc, DevRbspInst rb, const uint32_t *queue,
                                                                                                 const uint32_t *countPtr, uint32_t countImm, RayStream rays,
                                                                                                 HitStream hits, uint8_t *occ, DevCounters *counters,
                                                                                                 uint4 *rayStats, uint32_t *workCounter) {
    __shared__ uint2 stackMem[HPRT_RBSPINST_LDS * HPRT_RBSPINST_BLOCK];     // [entry][thread]: {node, tPlane} or {leaf node, position}
    __shared__ float dirTab[3 * RBSP_MAX_DIRECTIONS];
    if (threadIdx.x < 3 * RBSP_MAX_DIRECTIONS) dirTab[threadIdx.x] = rb.dirs[threadIdx.x];
    __syncthreads();
    if constexpr (KD) {
        RbspKdInstStep step{dirTab, rb.M, rb.off, rb.mask, rb.kdCounters};
        bspinst_walk<ANY_HIT, COUNT, QUAD, HPRT_RBSPINST_LDS, HPRT_RBSPINST_BLOCK, RbspKdInstStep, true>(sc, rb.nodes, rb.primIdx, (const float4 *)rb.entries, rb.lo, rb.hi,
                                                                                                         step, queue, countPtr, countImm, rays, hits, occ, counters,
                                                                                                         rayStats, workCounter, stackMem);
    } else {
        RbspInstStep step{dirTab, rb.M, rb.off, rb.mask};
        bspinst_walk<ANY_HIT, COUNT, QUAD, HPRT_RBSPINST_LDS, HPRT_RBSPINST_BLOCK>(sc, rb.nodes, rb.primIdx, (const float4 *)rb.entries, rb.lo, rb.hi, step, queue,
                                                                                   countPtr, countImm, rays, hits, occ, counters, rayStats, workCounter, stackMem);
    }
}

void LaunchRbspInstTrace(hipStream_t st, const DevScene &sc, const DevRbspInst &rb, bool kdAware, bool anyHit, bool count, const uint32_t *queue,
                         const uint32_t *countPtr, uint32_t countImm, uint32_t gridItems, const RayStream &rays, const HitStream &hits,
                         uint8_t *occ, DevCounters *counters, uint32_t *workCounter, uint4 *rayStats) {
    LaunchTreeWalk<HPRT_RBSPINST_BLOCK, HPRT_RBSPINST_WAVES, HPRT_RBSPINST_QUAD_WAVES>(st, sc, anyHit, count, gridItems, workCounter, [&](dim3 grid, dim3 block, auto a, auto c, auto q) {
        if (kdAware)
            hipLaunchKernelGGL((k_rbspinstwalk<decltype(a)::value, decltype(c)::value, decltype(q)::value, true>), grid, block, 0, st, sc, rb, queue, countPtr,
                               countImm, rays, hits, occ, counters, rayStats, workCounter);
        else
            hipLaunchKernelGGL((k_rbspinstwalk<decltype(a)::value, decltype(c)::value, decltype(q)::value, false>), grid, block, 0, st, sc, rb, queue, countPtr,
                               countImm, rays, hits, occ, counters, rayStats, workCounter);
    });
}

}  // namespace hprt
