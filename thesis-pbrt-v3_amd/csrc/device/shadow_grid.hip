// hprt device side — k_shadow_grid: the any-hit answer of point-light shadow rays from a light-centred candidate grid
// (../shadow_grid.h) instead of a BVH walk.
//
// BVHAccel::IntersectP(ray) is true if and only if some primitive p reports a hit AND the exact box of p's leaf passes
// Bounds3::IntersectP against the ray (kernels.hip, k_walk4: tMax never shrinks for an any-hit ray, so a leaf comes up exactly
// when its own box passes).  Nothing in that depends on the tree.  Every ray here ends at the light, so the triangles that can
// report a hit are listed — a superset, by the margins of the host build — in the cell of the grid that the ray's direction
// falls into, nearest to the light first; the kernel runs the walk's own tri_test over that list and, on a reported hit, the
// walk's own leaf-box test (slab_test on the min / max of the vertices for a one-triangle leaf, else on DevScene::leafBox).
//
// The lists are read from the grid's device image (../shadow_grid.h, ShadowGridImage): a 128-byte block per cell that holds the
// list's head and its first two candidates, vertices and all, and 48-byte records in list order for the rest, so that a ray's
// typical two or three candidates cost two or three 128-byte lines and as many dependent rounds.  DevScene::tris is not read.
//
// The lane machine that reads the lists is shared with k_distant_grid: grid_lanes.h (states, entry-word tests, launch sizing) and
// grid_lanes_body.h (the loop, with its description).  This file holds what is the point light's own: the cell of a direction.
#include "shadow_grid.h"
#include "dev_intersect.h"
#include "grid_lanes.h"

namespace hprt {

// workgroups of 256 threads per CU = waves per SIMD the kernel is compiled for; no LDS, no scratch.  The kernel fits seven (it needs
// 70 registers; eight, 64 registers, spills four), but its lanes gather 48-byte records from all over the triangle array, and more
// waves per CU only evict each other's lines: on the atrium's shadow rays five measured fastest (profiles/shadow_grid_ab.txt:
// seven and four 7-9 % slower, three 25 %).
#ifndef HPRT_SHADOW_GRID_WAVES
#define HPRT_SHADOW_GRID_WAVES 5
#endif

// The cell of a ray's direction as seen from the light (-d), and the sixteenth of the cell it falls into (*sub = su | sv << 4): the
// major axis is the largest |component|, ties to the lower axis; face = 2 axis + (negative side); (u, v) = the two other
// components, in cyclic order, over the major one's magnitude; a face side holds 16 R fine columns, floor((u + 1) 8 R).
// The host covers every fine column this can return for a ray that can report a hit (shadow_grid.cpp: the rectangle of a
// triangle's projection, widened by its margin, through the same expression in double).
__device__ __forceinline__ uint32_t sg_cell(vec3 d, uint32_t R, float fineScale, uint32_t *sub) {
    const float x = -d.x, y = -d.y, z = -d.z;
    const float ax = fabsf(x), ay = fabsf(y), az = fabsf(z);
    const bool a0 = ax >= ay && ax >= az, a1 = !a0 && ay >= az;
    const float mj = a0 ? x : a1 ? y : z, a = a0 ? y : a1 ? z : x, b = a0 ? z : a1 ? x : y;
    const float m = fabsf(mj);
    const float u = a / m, v = b / m;
    int fu = (int)floorf((u + 1.f) * fineScale), fv = (int)floorf((v + 1.f) * fineScale);
    fu = sel_max(0, sel_min(16 * (int)R - 1, fu)); fv = sel_max(0, sel_min(16 * (int)R - 1, fv));
    const uint32_t face = (a0 ? 0u : a1 ? 2u : 4u) + (mj < 0 ? 1u : 0u);
    *sub = ((uint32_t)fu & 15u) | (((uint32_t)fv & 15u) << 4);
    return (face * R + ((uint32_t)fv >> 4)) * R + ((uint32_t)fu >> 4);
}

__global__ __launch_bounds__(HPRT_TRACE_BLOCK, HPRT_SHADOW_GRID_WAVES)
void k_shadow_grid(DevScene sc, DevShadowGrid g, const uint32_t *queue, const uint32_t *countPtr, uint32_t countImm, RayStream rays, uint8_t *occ,
                   uint32_t *workCounter, uint32_t chunk, uint32_t refillMin) {
#define GRID_LANES_SETUP const float fineScale = 8.f * (float)g.R;
    // an entry is tested while key <= |d|^2 (1 + 2^-20): a hit lies between the origin and the light (tMax <= 1), so no farther from
    // the light than the origin.  (A caller's ray with tMax > 1 reads its lists to the end.)
#define GRID_LANES_RAY \
            const float dist2 = d.x * d.x + d.y * d.y + d.z * d.z; \
            lim = rayTMax <= 1.f ? dist2 * (1.f + 0x1p-20f) : HPRT_INF; \
            cell = sg_cell(d, g.R, fineScale, &sub);
#include "grid_lanes_body.h"
}

void LaunchShadowGrid(hipStream_t st, const DevScene &sc, const DevShadowGrid &g, const uint32_t *queue, const uint32_t *countPtr,
                      uint32_t countImm, uint32_t gridItems, const RayStream &rays, uint8_t *occ, uint32_t *workCounter) {
    if (gridItems == 0) return;
    (void)hipMemsetAsync(workCounter, 0, sizeof(uint32_t), st);
    static const uint32_t perCu = [] { const char *e = getenv("HPRT_SHADOW_GRID_PER_CU"); return e ? (uint32_t)std::min((int)HPRT_SHADOW_GRID_WAVES, std::max(1, atoi(e))) : (uint32_t)HPRT_SHADOW_GRID_WAVES; }();
    static const uint32_t refillMin = [] { const char *e = getenv("HPRT_SHADOW_GRID_REFILL"); return e ? (uint32_t)std::min(64, std::max(1, atoi(e))) : 32u; }();      // (idle lanes that start a refill: 32 measured 3-4 % faster than 8)
    const GridLaunchSize z = grid_launch_size(gridItems, perCu);
    hipLaunchKernelGGL(k_shadow_grid, dim3(z.blocks), dim3(HPRT_TRACE_BLOCK), 0, st, sc, g, queue, countPtr, countImm, rays, occ, workCounter, z.chunk, refillMin);
}

}  // namespace hprt
