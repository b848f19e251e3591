// hprt device side — k_distant_grid: the any-hit answer of distant-light shadow rays from a light-aligned candidate grid
// (../distant_grid.h) instead of a BVH walk.  lib/libhprt_dg.so: a library of its own beside libhprt.so.
//
// The argument is k_shadow_grid's (shadow_grid.hip): BVHAccel::IntersectP(ray) is true if and only if some primitive
// reports a hit AND the exact box of its leaf passes Bounds3::IntersectP, whatever structure names the primitives.  Every ray here
// runs along the light's direction w, so seen along w it is (almost) the point its origin projects to: the triangles that can
// report a hit are listed — a superset, by the margins of the host build — in the cell of that point, highest along w first, and
// the kernel runs the walk's own tri_test over the list and, on a reported hit, the walk's own leaf-box test.
//
// The machine is k_shadow_grid's, state for state: the same device image (a 128-byte block per cell with the list's first two
// candidates, 48-byte records for the rest), persistent waves with the walks' chunked dequeue and entry window, one round of loads
// per iteration for all lanes' states, one tri_test per iteration.  Only the step that takes in a ray differs: cell and sixteenth
// from the origin's two scalar products with the frame, the key limit from its height along w.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include "distant_grid.h"
#include "dev_intersect.h"

namespace hprt {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

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
// the ray's sixteenth lies in the part of the cell an entry's triangle reaches (shadow_grid.h: the lower 16 bits of the entry's second word)
__device__ __forceinline__ bool dg_reaches(uint32_t w, uint32_t sub) {
    const uint32_t su = sub & 15u, sv = sub >> 4;
    return su >= (w & 15u) && su <= ((w >> 4) & 15u) && sv >= ((w >> 8) & 15u) && sv <= ((w >> 12) & 15u);
}

__device__ __forceinline__ float dg_key(uint32_t w) { return __uint_as_float(w & SG_KEY_MASK); }

// DG_BLOCK: the first four words of the cell's block wanted (its head, triangle 0, the key words of entries 1 and 2); DG_BLOCK2: the
// block's triangle 1; DG_OVER: the 48-byte record of entry i (the near list, a cell's list from its third entry on)
enum : int { DG_IDLE = 0, DG_RAY = 1, DG_BLOCK = 2, DG_BLOCK2 = 3, DG_OVER = 4, DG_BOX = 5 };

__global__ __launch_bounds__(HPRT_TRACE_BLOCK, HPRT_DISTANT_GRID_WAVES)
void k_distant_grid(DevScene sc, DevDistantGrid g, const uint32_t *queue, const uint32_t *countPtr, uint32_t countImm, RayStream rays, uint8_t *occ,
                   uint32_t *workCounter, uint32_t chunk, uint32_t refillMin) {
    const uint32_t n = countPtr ? *countPtr : countImm;
    const uint32_t lane = __lane_id();
    const auto boxRsrc = __builtin_amdgcn_make_buffer_rsrc((void *)sc.leafBox, 0, (int)(sc.nPrims * 32u), 0x00020000);
    const auto imgRsrc = __builtin_amdgcn_make_buffer_rsrc((void *)g.image, 0, (int)g.imageBytes, 0x00020000);      // (blocks, then records: one resource, 32-bit byte offsets)
    const float robust = 1 + 2 * gamma_n(3);
    // the frame is uniform: U, the origins and the scales stay in scalar registers; V, W and hTop are moved to vector registers, of
    // which the kernel has a dozen to spare where the scalar file is full (102)
    float Vx = g.f.V[0], Vy = g.f.V[1], Vz = g.f.V[2], Wx = g.f.W[0], Wy = g.f.W[1], Wz = g.f.W[2], hTop = g.f.hTop;
    asm volatile("" : "+v"(Vx), "+v"(Vy), "+v"(Vz), "+v"(Wx), "+v"(Wy), "+v"(Wz), "+v"(hTop));
    int st = DG_IDLE;
    bool hit = false;
    uint32_t slot = 0u;
    // the list being read (the near list comes first, then the cell's): entry i of cnt is the one wanted or under test; recAt: the byte
    // offset of entry i's record (a cell's list: of entry 2's while i < 2); kwN: DG_BLOCK2, the key word of entry 2
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
        const unsigned long long idle = __ballot(st == DG_IDLE);
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
            if (st == DG_IDLE) {
                const uint32_t idx = base + rank;
                if (idx < localEnd) { slot = queue ? slotW : idx; hit = false; st = DG_RAY; }
            }
        }
        if (__ballot(st != DG_IDLE) == 0ull) {
            if (!moreWork) break;
            continue;
        }
        // ---- the loads of every lane's state, issued together ----
        u32x4 r0 = {0u, 0u, 0u, 0u}, r1 = {0u, 0u, 0u, 0u}, r2 = {0u, 0u, 0u, 0u};
        u32x4 r3 = {0u, 0u, 0u, 0u};
        if (st == DG_RAY) {
            r0 = __builtin_bit_cast(u32x4, rays.a[slot]);
            r1 = __builtin_bit_cast(u32x4, rays.b[slot]);
        } else if (st == DG_BOX) {
            const uint32_t pi = ePrim & SG_PRIM_MASK;
            r0 = __builtin_amdgcn_raw_buffer_load_b128(boxRsrc, pi * 32u, 0, 0);
            r1 = __builtin_amdgcn_raw_buffer_load_b128(boxRsrc, pi * 32u + 16u, 0, 0);
        } else if (st != DG_IDLE) {
            // a triangle with the words in its fourth lanes always arrives in r0 - r2: the block's first, its second, a record's
            const uint32_t at = st == DG_BLOCK ? cell * 128u + 16u : st == DG_BLOCK2 ? cell * 128u + 64u : recAt;
            r0 = __builtin_amdgcn_raw_buffer_load_b128(imgRsrc, at, 0, 0);
            r1 = __builtin_amdgcn_raw_buffer_load_b128(imgRsrc, at + 16u, 0, 0);
            r2 = __builtin_amdgcn_raw_buffer_load_b128(imgRsrc, at + 32u, 0, 0);
            if (st == DG_BLOCK) r3 = __builtin_amdgcn_raw_buffer_load_b128(imgRsrc, cell * 128u, 0, 0);
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
        if (st0 == DG_RAY) {
            ro = vec3(__uint_as_float(r0.x), __uint_as_float(r0.y), __uint_as_float(r0.z));
            rayTMax = __uint_as_float(r0.w);
            const vec3 d(__uint_as_float(r1.x), __uint_as_float(r1.y), __uint_as_float(r1.z));
            invDir = vec3(1 / d.x, 1 / d.y, 1 / d.z);
            shear = ray_shear(d, invDir);
            // the origin seen along w: its cell and sixteenth, and its height.  An entry is tested while key <= hTop - height: a
            // hit lies no lower along w than the origin (tMax <= 1; a caller's ray with tMax > 1 reads its lists to the end)
            const float pu = ro.x * g.f.U[0] + ro.y * g.f.U[1] + ro.z * g.f.U[2];
            const float pv = ro.x * Vx + ro.y * Vy + ro.z * Vz;
            const float ph = ro.x * Wx + ro.y * Wy + ro.z * Wz;
            lim = rayTMax <= 1.f ? hTop - ph : HPRT_INF;
            const uint32_t fu = dg_fine(pu, g.f.u0, g.f.scaleU, g.R), fv = dg_fine(pv, g.f.v0, g.f.scaleV, g.R);
            sub = (fu & 15u) | ((fv & 15u) << 4);
            cell = (fv >> 4) * g.R + (fu >> 4);
            i = 0u;
            if (g.nNear != 0u) { nearList = true; cnt = g.nNear; recAt = g.recordsAt; st = DG_OVER; }
            else { nearList = false; st = DG_BLOCK; }
        } else if (st0 == DG_BLOCK) {
            // r3: the block's head {count, record of entry 2, prim[0], key[0]}.  (i == 1: back after a leaf box that failed entry 0's hit)
            cnt = r3.x; recAt = g.recordsAt + r3.y * 48u;
            if (i == 0u) {
                if (cnt == 0u || dg_key(r3.w) > lim) listEnd = true;
                else if (dg_reaches(r3.w, sub)) { doTest = true; ePrim = r3.z; }
            }
        } else if (st0 == DG_BLOCK2) {
            doTest = true;
        } else if (st0 == DG_OVER) {
            // a key beyond the ray's origin ends a cell's list (near-list keys are 0); an entry whose triangle does not reach the
            // ray's sixteenth of the cell is passed over
            if (dg_key(r1.w) > lim) listEnd = true;
            else if (dg_reaches(r1.w, sub)) { doTest = true; ePrim = r0.w; }
        } else if (st0 == DG_BOX) {
            if (leaf_reached(__uint_as_float(r0.x), __uint_as_float(r0.y), __uint_as_float(r0.z), __uint_as_float(r0.w), __uint_as_float(r1.x), __uint_as_float(r1.y))) { hit = true; done = true; }
            else {
                // on with the entry behind the one under test: the block again for its second, else a record
                ++i;
                if (nearList || i > 2u) recAt += 48u;
                if (!nearList && i < 2u) st = DG_BLOCK;
                else if (i >= cnt) listEnd = true;
                else st = DG_OVER;
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
        if (boxWanted) st = DG_BOX;
        else if (!done && !listEnd) {
            // entry i is done with: whether the next one concerns the ray is known from the words that came with this one
            if (st0 == DG_BLOCK) {
                i = 1u;
                if (cnt <= 1u || dg_key(r1.w) > lim) listEnd = true;
                else if (dg_reaches(r1.w, sub)) { st = DG_BLOCK2; ePrim = r0.w; kwN = r2.w; }
                else { i = 2u; if (cnt <= 2u || dg_key(r2.w) > lim) listEnd = true; else st = DG_OVER; }
            } else if (st0 == DG_BLOCK2) {
                i = 2u;
                if (cnt <= 2u || dg_key(kwN) > lim) listEnd = true; else st = DG_OVER;
            } else if (st0 == DG_OVER) {
                ++i; recAt += 48u;
                if (i >= cnt || dg_key(r2.w) > lim) listEnd = true;
            }
        }
        if (listEnd) {
            if (nearList) { nearList = false; i = 0u; st = DG_BLOCK; }      // the near list is through: the cell's
            else done = true;
        }
        if (done) { occ[slot] = hit ? 1 : 0; st = DG_IDLE; }
    }
}

void LaunchDistantGrid(hipStream_t st, const DevScene &sc, const DevDistantGrid &g, const uint32_t *queue, const uint32_t *countPtr,
                      uint32_t countImm, uint32_t gridItems, const RayStream &rays, uint8_t *occ, uint32_t *workCounter) {
    if (gridItems == 0) return;
    (void)hipMemsetAsync(workCounter, 0, sizeof(uint32_t), st);
    // persistent waves: as many workgroups per CU as the kernel is compiled for, never more than the rays need (HPRT_TRACE_MAX_BLOCKS
    // and HPRT_TRACE_CHUNK_MAX: the walks' test hooks, a handful of waves working through many queue chunks each)
    static const uint32_t blockCap = [] { const char *e = getenv("HPRT_TRACE_MAX_BLOCKS"); return e ? (uint32_t)std::max(1, atoi(e)) : 0xffffffffu; }();
    static const uint32_t chunkMax = [] { const char *e = getenv("HPRT_TRACE_CHUNK_MAX"); return e ? (uint32_t)atoi(e) : 512u; }();
    const uint32_t refillMin = 32u;      // idle lanes that start a refill: k_shadow_grid's measured setting, not swept for this kernel
    const uint32_t blocks = std::min((uint32_t)(((size_t)gridItems + HPRT_TRACE_BLOCK - 1) / HPRT_TRACE_BLOCK), std::min(256u * (uint32_t)HPRT_DISTANT_GRID_WAVES, blockCap));
    const uint32_t nWaves = blocks * (HPRT_TRACE_BLOCK / 64);
    uint32_t chunk = gridItems / (nWaves * 4u);
    chunk = std::max(64u, std::min(chunkMax, chunk)) & ~63u;
    hipLaunchKernelGGL(k_distant_grid, dim3(blocks), dim3(HPRT_TRACE_BLOCK), 0, st, sc, g, queue, countPtr, countImm, rays, occ, workCounter, chunk, refillMin);
}

}  // namespace hprt
