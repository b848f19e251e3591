// hprt device side — the kd-tree walk (gfx950, wave64): KdTreeAccel::Intersect / IntersectP
// (accelerators/kdtreeaccel.cpp:381-521) with the leaf loops of KdAccelNode::intersectLeaf / intersectPLeaf (:95-146),
// restated operation for operation, over the reference's own 8-byte node array (kd_walk.h, DevKd).
//
// One ray per lane; persistent waves draw 64 rays at a time from the queue head (one atomic per wave and draw), so the
// kernel consumes the wavefront's queues, ray streams and hit records exactly like k_trace and the render loop does not
// know which walk ran.
//
// Todo list.  Every pending entry belongs to a different interior level of the current path, so a ray never holds more
// entries than the tree has levels (<= KD_TODO_MAX = 64, pbrt's maxTodo; the attach step refuses deeper trees).  An entry is
// {node, tPlane} (8 bytes): tPlane is the popped tMin, and the tMax the reference stores with it is always the tPlane of the
// entry below it (or the root interval's t1 when there is none) — tMax changes only at a push, where it becomes that push's
// tPlane, and at a pop, where it returns to the value it had at the push — so it is re-read from there, bit for bit.
// The first KD_LDS entries live in LDS ([entry][thread]: a wave's 64 lanes touch 64 consecutive 8-byte words), the rest in
// the scene's deep-stack area in HBM ([entry][grid thread], DevScene::deepStack), which has room for 57 more.
//
// Built with -ffp-contract=off: every float operation is one IEEE rounding in the reference's order.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include "kd_walk.h"
#include "../kdtree_builder.h"

#ifndef HPRT_KD_LDS
#define HPRT_KD_LDS 8
#endif
#define HPRT_KD_BLOCK 256
// workgroups per CU (= waves per SIMD): six for the triangle-only kernels (<= 80 registers), four with the quadric code (its
// interval-arithmetic call needs up to 128)
#ifndef HPRT_KD_WAVES
#define HPRT_KD_WAVES 6
#endif
#define HPRT_KD_QUAD_WAVES 4

namespace hprt {

static_assert(HPRT_KD_LDS + HPRT_SPILL_STACK >= (int)KD_TODO_MAX, "LDS + deep-stack entries must hold the deepest tree attach accepts");
static_assert(HPRT_DEEP_THREADS >= 256u * HPRT_KD_BLOCK * HPRT_KD_WAVES, "the deep-stack area must cover the kd walk's grid");

// Bounds3::IntersectP(const Ray &, Float *hitt0, Float *hitt1) (core/geometry.h:1730-1751): the root interval.  (The
// two-pointer form, not the invDir / dirIsNeg form the BVH walks evaluate with slab_test: t0 starts at 0, t1 at ray.tMax.)
__device__ __forceinline__ bool kd_root_interval(const DevKd &kd, vec3 ro, vec3 rd, float rayTMax, float *hitt0, float *hitt1) {
    float t0 = 0, t1 = rayTMax;
    const float robust = 1 + 2 * gamma_n(3);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float invRayDir = 1 / rd.get(i);
        float tNear = (kd.lo[i] - ro.get(i)) * invRayDir;
        float tFar = (kd.hi[i] - ro.get(i)) * invRayDir;
        if (tNear > tFar) { const float s = tNear; tNear = tFar; tFar = s; }
        tFar *= robust;
        t0 = tNear > t0 ? tNear : t0;
        t1 = tFar < t1 ? tFar : t1;
        if (t0 > t1) return false;
    }
    *hitt0 = t0; *hitt1 = t1;
    return true;
}

// ANY_HIT: IntersectP; COUNT: counters and per-ray statistics; QUAD: the scene has spheres (the interval-arithmetic test is
// compiled in only then).
template <bool ANY_HIT, bool COUNT, bool QUAD>
__global__ __launch_bounds__(HPRT_KD_BLOCK, QUAD ? HPRT_KD_QUAD_WAVES : HPRT_KD_WAVES) void k_kdwalk(DevScene sc, DevKd kd, const uint32_t *queue, const uint32_t *countPtr,
                                                                         uint32_t countImm, RayStream rays, HitStream hits, uint8_t *occ,
                                                                         DevCounters *counters, uint4 *rayStats, uint32_t *workCounter) {
    __shared__ uint2 stackMem[HPRT_KD_LDS * HPRT_KD_BLOCK];     // [entry][thread]: {node, tPlane}
    uint2 *const ldsStack = &stackMem[threadIdx.x];
    auto deepSlot = [&](int entry) -> volatile uint2 * {
        return (volatile uint2 *)sc.deepStack + (size_t)(entry - HPRT_KD_LDS) * HPRT_DEEP_THREADS + (blockIdx.x * HPRT_KD_BLOCK + threadIdx.x);
    };
    auto readEntry = [&](int entry) -> uint2 {
        if (entry < HPRT_KD_LDS) return ldsStack[entry * HPRT_KD_BLOCK];
        const volatile uint2 *p = deepSlot(entry);
        return make_uint2(p->x, p->y);
    };
    const uint32_t n = countPtr ? *countPtr : countImm;
    const uint32_t lane = __lane_id();
    TraceCount cnt = {0u, 0u, 0u, 0u, 0u};     // fetched: nbNodeTraversals, entered: kdTreeNodeTraversals (interior), leaf: leaves
    while (true) {
        uint32_t base = 0u;
        if (lane == 0) base = atomicAdd(workCounter, 64u);
        base = __shfl(base, 0);
        if (base >= n) break;
        const uint32_t idx = base + lane;
        if (idx >= n) continue;
        const uint32_t slot = queue ? queue[idx] : idx;
        const float4 ra = rays.a[slot], rb = rays.b[slot];
        const vec3 ro(ra.x, ra.y, ra.z), rd(rb.x, rb.y, rb.z);
        float rayTMax = ra.w;
        const TraceCount snap = cnt;
        bool hit = false;
        int32_t prim = -1; float hb0 = 0.f, hb1 = 0.f, hb2 = 0.f;
        float tMin, tMax;
        if (kd_root_interval(kd, ro, rd, rayTMax, &tMin, &tMax)) {
            const vec3 invDir(1 / rd.x, 1 / rd.y, 1 / rd.z);
            const RayShear shear = ray_shear(rd, invDir);
            const float rootTMax = tMax;
            int sp = 0;
            uint32_t node = 0u;
            bool done = false;
            while (!done) {
                if (!ANY_HIT && rayTMax < tMin) break;      // a hit closer than the current node
                if (COUNT) ++cnt.fetched;
                const uint2 nd = kd.nodes[node];
                if ((nd.y & 3u) != 3u) {
                    if (COUNT) ++cnt.entered;
                    const uint32_t axis = nd.y & 3u;
                    const float split = __uint_as_float(nd.x);
                    const float oA = axis == 0 ? ro.x : (axis == 1 ? ro.y : ro.z);
                    const float dA = axis == 0 ? rd.x : (axis == 1 ? rd.y : rd.z);
                    const float iA = axis == 0 ? invDir.x : (axis == 1 ? invDir.y : invDir.z);
                    const float tPlane = (split - oA) * iA;                    // planeDistance (core/geometry.h:1833-1835)
                    const bool belowFirst = (oA < split) || (oA == split && dA <= 0);
                    const uint32_t above = nd.y >> 2;
                    const uint32_t first = belowFirst ? node + 1u : above, second = belowFirst ? above : node + 1u;
                    if (tPlane > tMax || tPlane <= 0) node = first;
                    else if (tPlane < tMin) node = second;
                    else {
                        const uint2 e = make_uint2(second, __float_as_uint(tPlane));
                        if (sp < HPRT_KD_LDS) ldsStack[sp * HPRT_KD_BLOCK] = e;
                        else { volatile uint2 *p = deepSlot(sp); p->x = e.x; p->y = e.y; }
                        ++sp;
                        node = first;
                        tMax = tPlane;
                    }
                } else {
                    if (COUNT) ++cnt.leaf;
                    const uint32_t np = nd.y >> 2;
                    for (uint32_t i = 0; i < np; ++i) {
                        const uint32_t pi = np == 1u ? nd.x : kd.primIdx[nd.x + i];
                        const float4 v0 = sc.tris[3 * pi], v1 = sc.tris[3 * pi + 1], v2 = sc.tris[3 * pi + 2];
                        const uint32_t tag = __float_as_uint(v0.w);
                        if ((tag & TAG_KIND_MASK) == 0u) {
                            if (COUNT) ++cnt.tri;
                            float b0, b1, b2, t;
                            if (tri_test(vec3(v0.x, v0.y, v0.z), vec3(v1.x, v1.y, v1.z), vec3(v2.x, v2.y, v2.z), ro, rayTMax, shear, &b0, &b1, &b2, &t)) {
                                if (ANY_HIT) { hit = true; done = true; break; }
                                // a zero-area triangle reports no hit to Intersect (shapes/triangle.cpp:309-316), IntersectP does
                                if (!(tag & TAG_BOGUS)) { hit = true; rayTMax = t; prim = (int32_t)(pi | ((tag & TAG_BIN_MASK) << 24)); hb0 = b0; hb1 = b1; hb2 = b2; }
                            }
                        } else if (QUAD) {
                            if (COUNT) ++cnt.sphere;
                            const uint32_t si = __float_as_uint(v2.w);
                            DRay rr; rr.o = ro; rr.d = rd; rr.tMax = rayTMax;
                            DRay robj; vec3 ph; float phi, t;
                            // the exact pre-test (dev_intersect.h) settles most rays; the interval arithmetic runs for the rest
                            if (sphere_may_hit(sc.spheres[si], rr) && sphere_test(sc.spheres[si], rr, &robj, &ph, &phi, &t)) {
                                if (ANY_HIT) { hit = true; done = true; break; }
                                const uint32_t bin = (tag & TAG_BIN_MASK) == (BIN_TEXTURED << TAG_BIN_SHIFT) ? BIN_TEXTURED : BIN_GENERIC;
                                hit = true; rayTMax = t; prim = (int32_t)(pi | (bin << HIT_BIN_SHIFT)); hb0 = hb1 = hb2 = 0.f;
                            }
                        }
                    }
                    if (done) break;
                    if (sp == 0) break;
                    --sp;
                    const uint2 e = readEntry(sp);
                    node = e.x;
                    tMin = __uint_as_float(e.y);
                    tMax = sp > 0 ? __uint_as_float(readEntry(sp - 1).y) : rootTMax;
                }
            }
        }
        if (COUNT && rayStats) rayStats[slot] = make_uint4(cnt.entered - snap.entered, cnt.leaf - snap.leaf, (cnt.tri + cnt.sphere) - (snap.tri + snap.sphere), 0u);
        if (ANY_HIT) occ[slot] = hit ? 1 : 0;
        else {
            hit_store(hits, slot, hit ? prim : -1, hb0, hb1, hb2, rayTMax, -1);
        }
    }
    if (COUNT) wave_count_add(counters, ANY_HIT, cnt);
}

void LaunchKdTrace(hipStream_t st, const DevScene &sc, const DevKd &kd, bool anyHit, bool count, const uint32_t *queue,
                   const uint32_t *countPtr, uint32_t countImm, uint32_t gridItems, const RayStream &rays, const HitStream &hits,
                   uint8_t *occ, DevCounters *counters, uint32_t *workCounter, uint4 *rayStats) {
    LaunchTreeWalk<HPRT_KD_BLOCK, HPRT_KD_WAVES, HPRT_KD_QUAD_WAVES>(st, sc, anyHit, count, gridItems, workCounter, [&](dim3 grid, dim3 block, auto a, auto c, auto q) {
        hipLaunchKernelGGL((k_kdwalk<decltype(a)::value, decltype(c)::value, decltype(q)::value>), grid, block, 0, st, sc, kd, queue, countPtr, countImm, rays,
                           hits, occ, counters, rayStats, workCounter);
    });
}

}  // namespace hprt
