// hprt device side — the body of a GenericBSP walk (Intersect / IntersectP of accelerators/genericBSP.h's trees) over the
// reference's 8-byte node arrays: the root interval, the todo list, the leaf loop, the hit word and the counters.  The RBSP walk
// (rbsp_walk.hip), the rbspkd walk (rbspkd_walk.hip), the bsppaper walk (bsppaper_walk.hip) and the bsppaperkd walk (bsppaperkd_walk.hip) instantiate it; the kd walk (kd_walk.hip) is the same loop written out,
// and stays so because moving it here changes its register allocation, and so its code object.  A walk passes its interior step in as `Step`:
//   bool leaf(uint32_t flags), uint32_t high(uint32_t flags)   (aboveChild / nPrimitives),
//   void plane(uint32_t flags, float split, vec3 ro, vec3 rd, vec3 invDir, float *tPlane, bool *belowFirst).
// KD_SHARE (the rbspkd walk) counts the interior nodes for which the step's `bool kd(uint32_t flags)` holds apart as well: per
// ray in rayStats.w (0 for every other walk) and per wave through `void kd_count_add(bool anyHit, uint32_t n)`.
// NODE_AXIS (the bsppaper walk) gives the step per-node data: the step's `float4 axis(uint32_t node)` is fetched for every node and
// passed to `void plane(float4 axis, uint32_t flags, ...)` in front of the other arguments — requested together with the node's
// 8-byte word (1), or only once the node has turned out to be interior (2), or only for the interior nodes for which the step's
// `bool has_axis(uint32_t flags)` holds (3, the bsppaperkd walk: its kd nodes have none; `plane` gets zeros there).  0: the step
// has no per-node data (every other walk).
// (The step keeps no per-ray state: values that must survive the sphere test's call would cost scratch.)
//
// One ray per lane; persistent waves draw 64 rays at a time from the queue head (one atomic per wave and draw), so the kernels
// consume the wavefront's queues, ray streams and hit records exactly like k_trace and the render loop does not know which
// walk ran.
//
// Todo list.  Every pending entry belongs to a different interior level of the current path, so a ray never holds more
// entries than the tree has levels (<= 64, pbrt's maxTodo; the attach steps refuse deeper trees).  An entry is {node, tPlane}
// (8 bytes): tPlane is the popped tMin, and the tMax the reference stores with it is always the tPlane of the entry below it
// (or the root interval's t1 when there is none) — tMax changes only at a push, where it becomes that push's tPlane, and at a
// pop, where it returns to the value it had at the push — so it is re-read from there, bit for bit.  The first LDS entries
// live in LDS ([entry][thread]: a wave's 64 lanes touch 64 consecutive 8-byte words), the rest in the scene's deep-stack area
// in HBM ([entry][grid thread], DevScene::deepStack).
#pragma once
#include <hip/hip_runtime.h>
#include "kernels.h"

namespace hprt {

// Bounds3::IntersectP(const Ray &, Float *hitt0, Float *hitt1) (core/geometry.h:1730-1751): the root interval.  (The
// two-pointer form, not the invDir / dirIsNeg form the BVH walks evaluate with slab_test: t0 starts at 0, t1 at ray.tMax.)
__device__ __forceinline__ bool bsp_root_interval(const float *lo, const float *hi, vec3 ro, vec3 rd, float rayTMax, float *hitt0, float *hitt1) {
    float t0 = 0, t1 = rayTMax;
    const float robust = 1 + 2 * gamma_n(3);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float invRayDir = 1 / rd.get(i);
        float tNear = (lo[i] - ro.get(i)) * invRayDir;
        float tFar = (hi[i] - ro.get(i)) * invRayDir;
        if (tNear > tFar) { const float s = tNear; tNear = tFar; tFar = s; }
        tFar *= robust;
        t0 = tNear > t0 ? tNear : t0;
        t1 = tFar < t1 ? tFar : t1;
        if (t0 > t1) return false;
    }
    *hitt0 = t0; *hitt1 = t1;
    return true;
}

// The whole kernel body.  ANY_HIT: IntersectP (no early-out on a closer hit); COUNT: counters and per-ray statistics; QUAD:
// the scene has spheres.  nodes / primIdx: the attached tree (one-primitive leaves and primIdx hold ORDERED indices); lo / hi:
// GenericBSP::bounds.  stackMem: the kernel's [LDS][BLOCK] LDS todo entries.
template <bool ANY_HIT, bool COUNT, bool QUAD, int LDS, int BLOCK, class Step, bool KD_SHARE = false, int NODE_AXIS = 0>
__device__ __forceinline__ void bsp_walk(const DevScene &sc, const uint2 *nodes, const uint32_t *primIdx, const float *lo, const float *hi, Step &step,
                                         const uint32_t *queue, const uint32_t *countPtr, uint32_t countImm, const RayStream &rays,
                                         const HitStream &hits, uint8_t *occ, DevCounters *counters, uint4 *rayStats, uint32_t *workCounter,
                                         uint2 *stackMem) {
    uint2 *const ldsStack = &stackMem[threadIdx.x];
    auto deepSlot = [&](int entry) -> volatile uint2 * {
        return (volatile uint2 *)sc.deepStack + (size_t)(entry - LDS) * HPRT_DEEP_THREADS + (blockIdx.x * BLOCK + threadIdx.x);
    };
    auto readEntry = [&](int entry) -> uint2 {
        if (entry < LDS) return ldsStack[entry * BLOCK];
        const volatile uint2 *p = deepSlot(entry);
        return make_uint2(p->x, p->y);
    };
    const uint32_t n = countPtr ? *countPtr : countImm;
    const uint32_t lane = __lane_id();
    TraceCount cnt = {0u, 0u, 0u, 0u, 0u};     // fetched: nbNodeTraversals, entered: interior nodes, leaf: leaves
    uint32_t kdCnt = 0u;                       // KD_SHARE: of the entered interior nodes, kd ones
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
        const uint32_t kdSnap = kdCnt;
        bool hit = false;
        int32_t prim = -1; float hb0 = 0.f, hb1 = 0.f, hb2 = 0.f;
        float tMin, tMax;
        if (bsp_root_interval(lo, hi, ro, rd, rayTMax, &tMin, &tMax)) {
            const vec3 invDir(1 / rd.x, 1 / rd.y, 1 / rd.z);
            const RayShear shear = ray_shear(rd, invDir);
            const float rootTMax = tMax;
            int sp = 0;
            uint32_t node = 0u;
            bool done = false;
            while (!done) {
                if (!ANY_HIT && rayTMax < tMin) break;      // a hit closer than the current node
                if (COUNT) ++cnt.fetched;
                uint2 nd = nodes[node];
                [[maybe_unused]] float4 axis;
                if constexpr (NODE_AXIS == 1) {
                    axis = step.axis(node);
                    // an empty asm that takes the node word and the whole entry: both requests are issued before one wait, the
                    // entry as one 16-byte load, where the compiler would otherwise split it and sink the pieces into the branches
                    // that read them (the form of 2)
                    asm volatile("" : "+v"(nd.x), "+v"(nd.y), "+v"(axis.x), "+v"(axis.y), "+v"(axis.z), "+v"(axis.w));
                }
                if (!step.leaf(nd.y)) {
                    if (COUNT) ++cnt.entered;
                    if constexpr (COUNT && KD_SHARE) kdCnt += step.kd(nd.y) ? 1u : 0u;
                    float tPlane; bool belowFirst;
                    if constexpr (NODE_AXIS == 2) axis = step.axis(node);
                    if constexpr (NODE_AXIS == 3) { axis = make_float4(0.f, 0.f, 0.f, 0.f); if (step.has_axis(nd.y)) axis = step.axis(node); }
                    if constexpr (NODE_AXIS != 0) step.plane(axis, nd.y, __uint_as_float(nd.x), ro, rd, invDir, &tPlane, &belowFirst);
                    else step.plane(nd.y, __uint_as_float(nd.x), ro, rd, invDir, &tPlane, &belowFirst);
                    const uint32_t above = step.high(nd.y);
                    const uint32_t first = belowFirst ? node + 1u : above, second = belowFirst ? above : node + 1u;
                    if (tPlane > tMax || tPlane <= 0) node = first;
                    else if (tPlane < tMin) node = second;
                    else {
                        const uint2 e = make_uint2(second, __float_as_uint(tPlane));
                        if (sp < LDS) ldsStack[sp * BLOCK] = e;
                        else { volatile uint2 *p = deepSlot(sp); p->x = e.x; p->y = e.y; }
                        ++sp;
                        node = first;
                        tMax = tPlane;
                    }
                } else {
                    if (COUNT) ++cnt.leaf;
                    const uint32_t np = step.high(nd.y);
                    for (uint32_t i = 0; i < np; ++i) {
                        const uint32_t pi = np == 1u ? nd.x : primIdx[nd.x + i];
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
        if (COUNT && rayStats) rayStats[slot] = make_uint4(cnt.entered - snap.entered, cnt.leaf - snap.leaf, (cnt.tri + cnt.sphere) - (snap.tri + snap.sphere),
                                                    KD_SHARE ? kdCnt - kdSnap : 0u);
        if (ANY_HIT) occ[slot] = hit ? 1 : 0;
        else {
            hit_store(hits, slot, hit ? prim : -1, hb0, hb1, hb2, rayTMax, -1);
        }
    }
    if (COUNT) wave_count_add(counters, ANY_HIT, cnt);
    if constexpr (COUNT && KD_SHARE) step.kd_count_add(ANY_HIT, kdCnt);
}

}  // namespace hprt
