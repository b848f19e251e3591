// hprt device side — the rbspkd walk (gfx950, wave64): RBSPKd::Intersect / IntersectP (accelerators/rbspKd.cpp:490-638) with
// RBSPKdNode::intersectInterior (:69-92), restated operation for operation over the RBSP tree's 8-byte node array (rbsp_walk.h,
// DevRbsp).  The loop, the todo list and the leaf loop are bsp_walk (bsp_walk.h) with its kd share counted; this file holds the
// interior step and the per-pixel accumulation of that share.
//
// Interior step.  Axis nodes (direction < 3) take the kd form, planeDistance(split, ray, invDir, axis):
//   tPlane = (split - o[axis]) * invDir[axis],  belowFirst = o[axis] < split || (o[axis] == split && d[axis] <= 0);
// oblique nodes the RBSP walk's full dot products (rbsp_walk.hip).  The two forms differ where a component is +-inf, NaN or -0
// (DESIGN.md §8b), so the axis form reads ray.d[axis] — not invDir[axis], which is +0 for d = +inf.  Both are evaluated and the
// operands selected (no divergent branch): o / invDir / d [axis] are picked by comparisons, never by a runtime index, so no
// per-ray array lands in scratch.
//
// Built with -ffp-contract=off: every float operation is one IEEE rounding in the reference's order.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "rbspkd_walk.h"
#include "bsp_walk.h"
#include "../rbsp_builder.h"

#ifndef HPRT_RBSPKD_LDS
#define HPRT_RBSPKD_LDS 8
#endif
#define HPRT_RBSPKD_BLOCK 256
// workgroups per CU (= waves per SIMD): as for the RBSP walk, six for the triangle-only kernels, four with the quadric code
#define HPRT_RBSPKD_WAVES 6
#define HPRT_RBSPKD_QUAD_WAVES 4

namespace hprt {

static_assert(HPRT_RBSPKD_LDS + HPRT_SPILL_STACK >= (int)RBSP_TODO_MAX, "LDS + deep-stack entries must hold the deepest tree attach accepts");
static_assert(HPRT_DEEP_THREADS >= 256u * HPRT_RBSPKD_BLOCK * HPRT_RBSPKD_WAVES, "the deep-stack area must cover the rbspkd walk's grid");

struct RbspKdStep {
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

// ANY_HIT: IntersectP; COUNT: counters and per-ray statistics (with the kd share); QUAD: the scene has spheres.
template <bool ANY_HIT, bool COUNT, bool QUAD>
__global__ __launch_bounds__(HPRT_RBSPKD_BLOCK, QUAD ? HPRT_RBSPKD_QUAD_WAVES : HPRT_RBSPKD_WAVES) void k_rbspkdwalk(DevScene sc, DevRbspKd rb, const uint32_t *queue,
                                                                                         const uint32_t *countPtr, uint32_t countImm, RayStream rays,
                                                                                         HitStream hits, uint8_t *occ, DevCounters *counters,
                                                                                         uint4 *rayStats, uint32_t *workCounter) {
    __shared__ uint2 stackMem[HPRT_RBSPKD_LDS * HPRT_RBSPKD_BLOCK];     // [entry][thread]: {node, tPlane}
    __shared__ float dirTab[3 * RBSP_MAX_DIRECTIONS];
    if (threadIdx.x < 3 * RBSP_MAX_DIRECTIONS) dirTab[threadIdx.x] = rb.t.dirs[threadIdx.x];
    __syncthreads();
    RbspKdStep step{dirTab, rb.t.M, rb.t.off, rb.t.mask, rb.kdCounters};
    bsp_walk<ANY_HIT, COUNT, QUAD, HPRT_RBSPKD_LDS, HPRT_RBSPKD_BLOCK, RbspKdStep, true>(sc, rb.t.nodes, rb.t.primIdx, rb.t.lo, rb.t.hi, step, queue,
                                                                                       countPtr, countImm, rays, hits, occ, counters, rayStats,
                                                                                       workCounter, stackMem);
}

static inline uint32_t rbspkd_blocks_for(size_t n, uint32_t bs) { return (uint32_t)((n + bs - 1) / bs); }

void LaunchRbspKdTrace(hipStream_t st, const DevScene &sc, const DevRbspKd &rb, bool anyHit, bool count, const uint32_t *queue,
                       const uint32_t *countPtr, uint32_t countImm, uint32_t gridItems, const RayStream &rays, const HitStream &hits,
                       uint8_t *occ, DevCounters *counters, uint32_t *workCounter, uint4 *rayStats) {
    LaunchTreeWalk<HPRT_RBSPKD_BLOCK, HPRT_RBSPKD_WAVES, HPRT_RBSPKD_QUAD_WAVES>(st, sc, anyHit, count, gridItems, workCounter, [&](dim3 grid, dim3 block, auto a, auto c, auto q) {
        hipLaunchKernelGGL((k_rbspkdwalk<decltype(a)::value, decltype(c)::value, decltype(q)::value>), grid, block, 0, st, sc, rb, queue, countPtr, countImm, rays,
                           hits, occ, counters, rayStats, workCounter);
    });
}

// k_pixel_stats (kernels.hip) for the kd share: the same ray -> pixel mapping, rayStats.w added to pixKd[anyHit][p]
__global__ __launch_bounds__(256) void k_pixel_kd_stats(const uint4 *rayStats, const float4 *ids, const uint32_t *queue, const uint32_t *countPtr,
                                                        uint32_t countImm, uint32_t nPix, int anyHit, uint32_t *pixKd) {
    const uint32_t n = countPtr ? *countPtr : countImm;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t slot = queue ? queue[i] : i;
    const uint32_t kd = rayStats[slot].w;
    const uint32_t p = (ids ? __float_as_uint(ids[slot].w) : slot) % nPix;      // ids == nullptr: camera rays, path id = slot
    if (kd) atomicAdd(pixKd + (anyHit ? nPix : 0u) + p, kd);
}
void LaunchPixelKdStats(hipStream_t st, const uint4 *rayStats, const float4 *ids, const uint32_t *queue, const uint32_t *countPtr,
                        uint32_t countImm, uint32_t gridItems, uint32_t nPix, bool anyHit, uint32_t *pixKd) {
    if (gridItems) hipLaunchKernelGGL(k_pixel_kd_stats, dim3(rbspkd_blocks_for(gridItems, 256)), dim3(256), 0, st, rayStats, ids, queue, countPtr, countImm,
                                      nPix, anyHit ? 1 : 0, pixKd);
}
__global__ __launch_bounds__(256) void k_pixel_kd_stats_to_film(const uint32_t *pixKd, const uint32_t *pixelXY, uint32_t nPix, int cx0, int cy0, int width,
                                                                size_t filmPixels, unsigned long long *out2) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nPix) return;
    const uint32_t pxy = pixelXY[p];
    const size_t f = (size_t)((int)(pxy >> 16) - cy0) * (size_t)width + (size_t)((int)(pxy & 0xffffu) - cx0);
    out2[f] = pixKd[p];
    out2[filmPixels + f] = pixKd[(size_t)nPix + p];
}
void LaunchPixelKdStatsToFilm(hipStream_t st, const uint32_t *pixKd, const uint32_t *pixelXY, uint32_t nPix, int cx0, int cy0, int width,
                              size_t filmPixels, unsigned long long *out2) {
    if (nPix) hipLaunchKernelGGL(k_pixel_kd_stats_to_film, dim3(rbspkd_blocks_for(nPix, 256)), dim3(256), 0, st, pixKd, pixelXY, nPix, cx0, cy0, width,
                                 filmPixels, out2);
}

}  // namespace hprt
