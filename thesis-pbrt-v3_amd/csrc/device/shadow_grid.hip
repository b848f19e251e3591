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
// Persistent waves with the walks' chunked dequeue and entry window.  A lane is a small state machine — ray wanted, block
// wanted, the block's second triangle wanted, a record wanted, leaf box wanted — and every iteration of the wave issues the
// loads of all its lanes' states together and waits once: a lane that starts a new ray costs the others no round trip of their own.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include "shadow_grid.h"
#include "dev_intersect.h"
#include "../shadow_grid.h"

namespace hprt {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

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
// the ray's sixteenth lies in the part of the cell an entry's triangle reaches (shadow_grid.h: the lower 16 bits of the entry's second word)
__device__ __forceinline__ bool sg_reaches(uint32_t w, uint32_t sub) {
    const uint32_t su = sub & 15u, sv = sub >> 4;
    return su >= (w & 15u) && su <= ((w >> 4) & 15u) && sv >= ((w >> 8) & 15u) && sv <= ((w >> 12) & 15u);
}

__device__ __forceinline__ float sg_key(uint32_t w) { return __uint_as_float(w & SG_KEY_MASK); }

// SG_BLOCK: the first four words of the cell's block wanted (its head, triangle 0, the key words of entries 1 and 2); SG_BLOCK2: the
// block's triangle 1; SG_OVER: the 48-byte record of entry i (the near list, a cell's list from its third entry on)
enum : int { SG_IDLE = 0, SG_RAY = 1, SG_BLOCK = 2, SG_BLOCK2 = 3, SG_OVER = 4, SG_BOX = 5 };

__global__ __launch_bounds__(HPRT_TRACE_BLOCK, HPRT_SHADOW_GRID_WAVES)
void k_shadow_grid(DevScene sc, DevShadowGrid g, const uint32_t *queue, const uint32_t *countPtr, uint32_t countImm, RayStream rays, uint8_t *occ,
                   uint32_t *workCounter, uint32_t chunk, uint32_t refillMin) {
    const uint32_t n = countPtr ? *countPtr : countImm;
    const uint32_t lane = __lane_id();
    const auto boxRsrc = __builtin_amdgcn_make_buffer_rsrc((void *)sc.leafBox, 0, (int)(sc.nPrims * 32u), 0x00020000);
    const auto imgRsrc = __builtin_amdgcn_make_buffer_rsrc((void *)g.image, 0, (int)g.imageBytes, 0x00020000);      // (blocks, then records: one resource, 32-bit byte offsets)
    const float robust = 1 + 2 * gamma_n(3);
    const float fineScale = 8.f * (float)g.R;
    int st = SG_IDLE;
    bool hit = false;
    uint32_t slot = 0u;
    // the list being read (the near list comes first, then the cell's): entry i of cnt is the one wanted or under test; recAt: the byte
    // offset of entry i's record (a cell's list: of entry 2's while i < 2); kwN: SG_BLOCK2, the key word of entry 2
    uint32_t i = 0u, cnt = 0u, recAt = 0u, kwN = 0u, cell = 0u;
    bool nearList = false;
    uint32_t ePrim = 0u;      // the candidate under test (entry i)
    uint32_t sub = 0u;        // the sixteenth of its cell the ray falls into
    vec3 ro, invDir;
    float rayTMax = 0.f, lim = 0.f;
    RayShear shear; shear.k0 = shear.k1 = false; shear.Sx = shear.Sy = shear.Sz = 0.f;
    bool moreWork = n > 0;
    uint32_t localNext = 0u, localEnd = 0u;
    uint32_t window = 0u, windowBase = 0xffffffffu;
    while (true) {
        // ---- idle lanes take the next rays of the queue (k_walk4's dequeue: chunks off the work counter, slots through the entry window) ----
        const unsigned long long idle = __ballot(st == SG_IDLE);
        if (moreWork && ((uint32_t)__popcll(idle) >= refillMin || idle == ~0ull)) {
            if (localNext >= localEnd) {
                uint32_t base = 0u;
                if (lane == 0) base = atomicAdd(workCounter, chunk);
                base = __builtin_amdgcn_readfirstlane(base);
                localNext = base < n ? base : n;
                localEnd = (base + chunk < n) ? base + chunk : n;
                if (localNext >= localEnd) moreWork = false;
                windowBase = 0xffffffffu;      // a new chunk: the window read ahead belongs to the old one
            }
            const uint32_t want = (uint32_t)__popcll(idle);
            const uint32_t base = localNext;
            localNext = (localNext + want < localEnd) ? localNext + want : localEnd;
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
            uint32_t slotW = 0u;
            if (queue) {
                if (windowBase != base) { window = (base + lane < localEnd) ? queue[base + lane] : 0u; windowBase = base; }
                slotW = __shfl(window, (int)rank);
                window = (localNext + lane < localEnd) ? queue[localNext + lane] : 0u;
                windowBase = localNext;
            }
            if (st == SG_IDLE) {
                const uint32_t idx = base + rank;
                if (idx < localEnd) { slot = queue ? slotW : idx; hit = false; st = SG_RAY; }
            }
        }
        if (__ballot(st != SG_IDLE) == 0ull) {
            if (!moreWork) break;
            continue;
        }
        // ---- the loads of every lane's state, issued together ----
        u32x4 r0 = {0u, 0u, 0u, 0u}, r1 = {0u, 0u, 0u, 0u}, r2 = {0u, 0u, 0u, 0u};
        u32x4 r3 = {0u, 0u, 0u, 0u};
        if (st == SG_RAY) {
            r0 = __builtin_bit_cast(u32x4, rays.a[slot]);
            r1 = __builtin_bit_cast(u32x4, rays.b[slot]);
        } else if (st == SG_BOX) {
            const uint32_t pi = ePrim & SG_PRIM_MASK;
            r0 = __builtin_amdgcn_raw_buffer_load_b128(boxRsrc, pi * 32u, 0, 0);
            r1 = __builtin_amdgcn_raw_buffer_load_b128(boxRsrc, pi * 32u + 16u, 0, 0);
        } else if (st != SG_IDLE) {
            // a triangle with the words in its fourth lanes always arrives in r0 - r2: the block's first, its second, a record's
            const uint32_t at = st == SG_BLOCK ? cell * 128u + 16u : st == SG_BLOCK2 ? cell * 128u + 64u : recAt;
            r0 = __builtin_amdgcn_raw_buffer_load_b128(imgRsrc, at, 0, 0);
            r1 = __builtin_amdgcn_raw_buffer_load_b128(imgRsrc, at + 16u, 0, 0);
            r2 = __builtin_amdgcn_raw_buffer_load_b128(imgRsrc, at + 32u, 0, 0);
            if (st == SG_BLOCK) r3 = __builtin_amdgcn_raw_buffer_load_b128(imgRsrc, cell * 128u, 0, 0);
        }
        asm volatile("" : "+v"(r0), "+v"(r1), "+v"(r2), "+v"(r3));
        // ---- one step of every lane ----
        // the leaf's own box, exactly, as k_walk4's leaf_reached evaluates it
        auto leaf_reached = [&](float lx, float ly, float lz, float hx, float hy, float hz) -> bool {
            float tEn;
            return slab_test(lx, hx, ly, hy, lz, hz, ro, invDir, invDir.x < 0, invDir.y < 0, invDir.z < 0, robust, &tEn) && tEn < rayTMax;
        };
        const int st0 = st;         // the state whose loads have arrived
        bool done = false;          // the ray's answer is known
        bool listEnd = false;       // the list being read holds nothing more for this ray
        bool doTest = false;        // r0 - r2 hold a candidate (ePrim) that the ray meets
        if (st0 == SG_RAY) {
            ro = vec3(__uint_as_float(r0.x), __uint_as_float(r0.y), __uint_as_float(r0.z));
            rayTMax = __uint_as_float(r0.w);
            const vec3 d(__uint_as_float(r1.x), __uint_as_float(r1.y), __uint_as_float(r1.z));
            invDir = vec3(1 / d.x, 1 / d.y, 1 / d.z);
            shear = ray_shear(d, invDir);
            // an entry is tested while key <= |d|^2 (1 + 2^-20): a hit lies between the origin and the light (tMax <= 1), so no
            // farther from the light than the origin.  (A caller's ray with tMax > 1 reads its lists to the end.)
            const float dist2 = d.x * d.x + d.y * d.y + d.z * d.z;
            lim = rayTMax <= 1.f ? dist2 * (1.f + 0x1p-20f) : HPRT_INF;
            cell = sg_cell(d, g.R, fineScale, &sub);
            i = 0u;
            if (g.nNear != 0u) { nearList = true; cnt = g.nNear; recAt = g.recordsAt; st = SG_OVER; }
            else { nearList = false; st = SG_BLOCK; }
        } else if (st0 == SG_BLOCK) {
            // r3: the block's head {count, record of entry 2, prim[0], key[0]}.  (i == 1: back after a leaf box that failed entry 0's hit)
            cnt = r3.x; recAt = g.recordsAt + r3.y * 48u;
            if (i == 0u) {
                if (cnt == 0u || sg_key(r3.w) > lim) listEnd = true;
                else if (sg_reaches(r3.w, sub)) { doTest = true; ePrim = r3.z; }
            }
        } else if (st0 == SG_BLOCK2) {
            doTest = true;
        } else if (st0 == SG_OVER) {
            // a key beyond the ray's origin ends a cell's list (near-list keys are 0); an entry whose triangle does not reach the
            // ray's sixteenth of the cell is passed over
            if (sg_key(r1.w) > lim) listEnd = true;
            else if (sg_reaches(r1.w, sub)) { doTest = true; ePrim = r0.w; }
        } else if (st0 == SG_BOX) {
            if (leaf_reached(__uint_as_float(r0.x), __uint_as_float(r0.y), __uint_as_float(r0.z), __uint_as_float(r0.w), __uint_as_float(r1.x), __uint_as_float(r1.y))) { hit = true; done = true; }
            else {
                // on with the entry behind the one under test: the block again for its second, else a record
                ++i;
                if (nearList || i > 2u) recAt += 48u;
                if (!nearList && i < 2u) st = SG_BLOCK;
                else if (i >= cnt) listEnd = true;
                else st = SG_OVER;
            }
        }
        bool boxWanted = false;
        if (doTest) {
            asm volatile("" : "+v"(r0), "+v"(r1), "+v"(r2));
            const vec3 p0(__uint_as_float(r0.x), __uint_as_float(r0.y), __uint_as_float(r0.z)), p1(__uint_as_float(r1.x), __uint_as_float(r1.y), __uint_as_float(r1.z)),
                       p2(__uint_as_float(r2.x), __uint_as_float(r2.y), __uint_as_float(r2.z));
            float b0, b1, b2, t;
            if (tri_test(p0, p1, p2, ro, rayTMax, shear, &b0, &b1, &b2, &t)) {
                // a hit counts if the reference's walk reaches this primitive's leaf
                if (ePrim & SG_SINGLE) {
                    if (leaf_reached(fminf(fminf(p0.x, p1.x), p2.x), fminf(fminf(p0.y, p1.y), p2.y), fminf(fminf(p0.z, p1.z), p2.z),
                                     fmaxf(fmaxf(p0.x, p1.x), p2.x), fmaxf(fmaxf(p0.y, p1.y), p2.y), fmaxf(fmaxf(p0.z, p1.z), p2.z))) { hit = true; done = true; }
                } else boxWanted = true;
            }
        }
        if (boxWanted) st = SG_BOX;
        else if (!done && !listEnd) {
            // entry i is done with: whether the next one concerns the ray is known from the words that came with this one
            if (st0 == SG_BLOCK) {
                i = 1u;
                if (cnt <= 1u || sg_key(r1.w) > lim) listEnd = true;
                else if (sg_reaches(r1.w, sub)) { st = SG_BLOCK2; ePrim = r0.w; kwN = r2.w; }
                else { i = 2u; if (cnt <= 2u || sg_key(r2.w) > lim) listEnd = true; else st = SG_OVER; }
            } else if (st0 == SG_BLOCK2) {
                i = 2u;
                if (cnt <= 2u || sg_key(kwN) > lim) listEnd = true; else st = SG_OVER;
            } else if (st0 == SG_OVER) {
                ++i; recAt += 48u;
                if (i >= cnt || sg_key(r2.w) > lim) listEnd = true;
            }
        }
        if (listEnd) {
            if (nearList) { nearList = false; i = 0u; st = SG_BLOCK; }      // the near list is through: the cell's
            else done = true;
        }
        if (done) { occ[slot] = hit ? 1 : 0; st = SG_IDLE; }
    }
}

void LaunchShadowGrid(hipStream_t st, const DevScene &sc, const DevShadowGrid &g, const uint32_t *queue, const uint32_t *countPtr,
                      uint32_t countImm, uint32_t gridItems, const RayStream &rays, uint8_t *occ, uint32_t *workCounter) {
    if (gridItems == 0) return;
    (void)hipMemsetAsync(workCounter, 0, sizeof(uint32_t), st);
    // persistent waves: as many workgroups per CU as the kernel is compiled for, never more than the rays need (HPRT_TRACE_MAX_BLOCKS
    // and HPRT_TRACE_CHUNK_MAX: the walks' test hooks, a handful of waves working through many queue chunks each)
    static const uint32_t blockCap = [] { const char *e = getenv("HPRT_TRACE_MAX_BLOCKS"); return e ? (uint32_t)std::max(1, atoi(e)) : 0xffffffffu; }();
    static const uint32_t perCu = [] { const char *e = getenv("HPRT_SHADOW_GRID_PER_CU"); return e ? (uint32_t)std::min((int)HPRT_SHADOW_GRID_WAVES, std::max(1, atoi(e))) : (uint32_t)HPRT_SHADOW_GRID_WAVES; }();
    static const uint32_t chunkMax = [] { const char *e = getenv("HPRT_TRACE_CHUNK_MAX"); return e ? (uint32_t)atoi(e) : 512u; }();
    static const uint32_t refillMin = [] { const char *e = getenv("HPRT_SHADOW_GRID_REFILL"); return e ? (uint32_t)std::min(64, std::max(1, atoi(e))) : 32u; }();      // (idle lanes that start a refill: 32 measured 3-4 % faster than 8)
    const uint32_t blocks = std::min((uint32_t)(((size_t)gridItems + HPRT_TRACE_BLOCK - 1) / HPRT_TRACE_BLOCK), std::min(256u * perCu, blockCap));
    const uint32_t nWaves = blocks * (HPRT_TRACE_BLOCK / 64);
    uint32_t chunk = gridItems / (nWaves * 4u);
    chunk = std::max(64u, std::min(chunkMax, chunk)) & ~63u;
    hipLaunchKernelGGL(k_shadow_grid, dim3(blocks), dim3(HPRT_TRACE_BLOCK), 0, st, sc, g, queue, countPtr, countImm, rays, occ, workCounter, chunk, refillMin);
}

}  // namespace hprt
