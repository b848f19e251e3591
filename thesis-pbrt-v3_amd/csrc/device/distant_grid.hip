// hprt device side — k_distant_grid: the any-hit answer of distant-light shadow rays from a light-aligned candidate grid
// (../distant_grid.h) instead of a BVH walk.  lib/libhprt_dg.so: a library of its own beside libhprt.so.
//
// The argument is k_shadow_grid's (shadow_grid.hip): BVHAccel::IntersectP(ray) is true if and only if some primitive
// reports a hit AND the exact box of its leaf passes Bounds3::IntersectP, whatever structure names the primitives.  Every ray here
// runs along the light's direction w, so seen along w it is (almost) the point its origin projects to: the triangles that can
// report a hit are listed — a superset, by the margins of the host build — in the cell of that point, highest along w first, and
// the kernel runs the walk's own tri_test over the list and, on a reported hit, the walk's own leaf-box test.
//
// The machine is k_shadow_grid's: grid_lanes.h and grid_lanes_body.h, over the same device image (a 128-byte block per cell with the
// list's first two candidates, 48-byte records for the rest).  Only the step that takes in a ray is this kernel's own: cell and
// sixteenth from the origin's two scalar products with the frame, the key limit from its height along w.
#include "distant_grid.h"
#include "dev_intersect.h"
#include "grid_lanes.h"

namespace hprt {

// workgroups of 256 threads per CU = waves per SIMD the kernel is compiled for, as k_shadow_grid (five measured fastest there: the
// kernel is bound by the bytes of its gathers); no LDS, no scratch, within the 96 registers of five.
#ifndef HPRT_DISTANT_GRID_WAVES
#define HPRT_DISTANT_GRID_WAVES 5
#endif

// The fine column of a projection: floor((p - x0) * scale), clamped to the 16 R columns of a side.  The host covers every column
// this can return for a ray that can report a hit (distant_grid.cpp: the same expression in double over the rectangle of a
// triangle's projection, widened by the margin).
__device__ __forceinline__ uint32_t dg_fine(float p, float x0, float scale, uint32_t R) {
    const int f = (int)floorf((p - x0) * scale);
    return (uint32_t)sel_max(0, sel_min(16 * (int)R - 1, f));
}

__global__ __launch_bounds__(HPRT_TRACE_BLOCK, HPRT_DISTANT_GRID_WAVES)
void k_distant_grid(DevScene sc, DevDistantGrid g, const uint32_t *queue, const uint32_t *countPtr, uint32_t countImm, RayStream rays, uint8_t *occ,
                   uint32_t *workCounter, uint32_t chunk, uint32_t refillMin) {
    // the frame is uniform: U, the origins and the scales stay in scalar registers; V, W and hTop are moved to vector registers, of
    // which the kernel has a dozen to spare where the scalar file is full (102)
#define GRID_LANES_SETUP \
    float Vx = g.f.V[0], Vy = g.f.V[1], Vz = g.f.V[2], Wx = g.f.W[0], Wy = g.f.W[1], Wz = g.f.W[2], hTop = g.f.hTop; \
    asm volatile("" : "+v"(Vx), "+v"(Vy), "+v"(Vz), "+v"(Wx), "+v"(Wy), "+v"(Wz), "+v"(hTop));
    // the origin seen along w: its cell and sixteenth, and its height.  An entry is tested while key <= hTop - height: a hit lies no
    // lower along w than the origin (tMax <= 1; a caller's ray with tMax > 1 reads its lists to the end)
#define GRID_LANES_RAY \
            const float pu = ro.x * g.f.U[0] + ro.y * g.f.U[1] + ro.z * g.f.U[2]; \
            const float pv = ro.x * Vx + ro.y * Vy + ro.z * Vz; \
            const float ph = ro.x * Wx + ro.y * Wy + ro.z * Wz; \
            lim = rayTMax <= 1.f ? hTop - ph : HPRT_INF; \
            const uint32_t fu = dg_fine(pu, g.f.u0, g.f.scaleU, g.R), fv = dg_fine(pv, g.f.v0, g.f.scaleV, g.R); \
            sub = (fu & 15u) | ((fv & 15u) << 4); \
            cell = (fv >> 4) * g.R + (fu >> 4);
#include "grid_lanes_body.h"
}

void LaunchDistantGrid(hipStream_t st, const DevScene &sc, const DevDistantGrid &g, const uint32_t *queue, const uint32_t *countPtr,
                      uint32_t countImm, uint32_t gridItems, const RayStream &rays, uint8_t *occ, uint32_t *workCounter) {
    if (gridItems == 0) return;
    (void)hipMemsetAsync(workCounter, 0, sizeof(uint32_t), st);
    const uint32_t refillMin = 32u;      // idle lanes that start a refill: k_shadow_grid's measured setting, not swept for this kernel
    const GridLaunchSize z = grid_launch_size(gridItems, (uint32_t)HPRT_DISTANT_GRID_WAVES);
    hipLaunchKernelGGL(k_distant_grid, dim3(z.blocks), dim3(HPRT_TRACE_BLOCK), 0, st, sc, g, queue, countPtr, countImm, rays, occ, workCounter, z.chunk, refillMin);
}

}  // namespace hprt
