// hprt device side — the RBSP walk (gfx950, wave64): RBSP::Intersect / IntersectP (accelerators/rbsp.cpp:405-547) with the leaf
// loops of RBSPNode::intersectLeaf / intersectPLeaf (:90-132), restated operation for operation, over the reference's own
// 8-byte node array (rbsp_walk.h, DevRbsp).  The loop, the todo list and the leaf loop are bsp_walk (bsp_walk.h); this file
// holds the interior step.
//
// Interior step (RBSPNode::intersectInterior, planeDistance, core/geometry.h:1837-1843): pO = Dot(dir, o) and
// iD = 1 / Dot(dir, d) as full float dot products for EVERY direction, the axis directions included: 1*o.x + 0*o.y + 0*o.z is
// not o.x when a component is +-inf or NaN or o.x = -0, and with d.x = -0 (d.y, d.z >= 0) 1 / Dot is +inf where kd's invDir.x
// is -inf, so rbsp-3 does not borrow the kd walk's component shortcut.  The direction table sits in LDS (3 * M floats per
// workgroup) and the two dot products are recomputed at every interior node: they are pure functions of the ray, so any
// placement gives the same bits, and this one needs no per-ray registers (a runtime-indexed per-ray array would live in
// scratch) — DESIGN.md §8b.
//
// Built with -ffp-contract=off: every float operation is one IEEE rounding in the reference's order.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "rbsp_walk.h"
#include "bsp_walk.h"
#include "../rbsp_builder.h"

#ifndef HPRT_RBSP_LDS
#define HPRT_RBSP_LDS 8
#endif
#define HPRT_RBSP_BLOCK 256
// workgroups per CU (= waves per SIMD): as for the kd walk, six for the triangle-only kernels, four with the quadric code
#ifndef HPRT_RBSP_WAVES
#define HPRT_RBSP_WAVES 6
#endif
#define HPRT_RBSP_QUAD_WAVES 4

namespace hprt {

static_assert(HPRT_RBSP_LDS + HPRT_SPILL_STACK >= (int)RBSP_TODO_MAX, "LDS + deep-stack entries must hold the deepest tree attach accepts");
static_assert(HPRT_DEEP_THREADS >= 256u * HPRT_RBSP_BLOCK * HPRT_RBSP_WAVES, "the deep-stack area must cover the RBSP walk's grid");

struct RbspStep {
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

// ANY_HIT: IntersectP; COUNT: counters and per-ray statistics; QUAD: the scene has spheres (the interval-arithmetic test is
// compiled in only then).
template <bool ANY_HIT, bool COUNT, bool QUAD>
__global__ __launch_bounds__(HPRT_RBSP_BLOCK, QUAD ? HPRT_RBSP_QUAD_WAVES : HPRT_RBSP_WAVES) void k_rbspwalk(DevScene sc, DevRbsp rb, const uint32_t *queue, const uint32_t *countPtr,
                                                                                 uint32_t countImm, RayStream rays, HitStream hits, uint8_t *occ,
                                                                                 DevCounters *counters, uint4 *rayStats, uint32_t *workCounter) {
    __shared__ uint2 stackMem[HPRT_RBSP_LDS * HPRT_RBSP_BLOCK];     // [entry][thread]: {node, tPlane}
    __shared__ float dirTab[3 * RBSP_MAX_DIRECTIONS];
    if (threadIdx.x < 3 * RBSP_MAX_DIRECTIONS) dirTab[threadIdx.x] = rb.dirs[threadIdx.x];
    __syncthreads();
    RbspStep step{dirTab, rb.M, rb.off, rb.mask};
    bsp_walk<ANY_HIT, COUNT, QUAD, HPRT_RBSP_LDS, HPRT_RBSP_BLOCK>(sc, rb.nodes, rb.primIdx, rb.lo, rb.hi, step, queue, countPtr, countImm, rays, hits,
                                                                   occ, counters, rayStats, workCounter, stackMem);
}

void LaunchRbspTrace(hipStream_t st, const DevScene &sc, const DevRbsp &rb, bool anyHit, bool count, const uint32_t *queue,
                     const uint32_t *countPtr, uint32_t countImm, uint32_t gridItems, const RayStream &rays, const HitStream &hits,
                     uint8_t *occ, DevCounters *counters, uint32_t *workCounter, uint4 *rayStats) {
    LaunchTreeWalk<HPRT_RBSP_BLOCK, HPRT_RBSP_WAVES, HPRT_RBSP_QUAD_WAVES>(st, sc, anyHit, count, gridItems, workCounter, [&](dim3 grid, dim3 block, auto a, auto c, auto q) {
        hipLaunchKernelGGL((k_rbspwalk<decltype(a)::value, decltype(c)::value, decltype(q)::value>), grid, block, 0, st, sc, rb, queue, countPtr, countImm, rays,
                           hits, occ, counters, rayStats, workCounter);
    });
}

}  // namespace hprt
