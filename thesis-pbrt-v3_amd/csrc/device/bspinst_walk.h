// hprt device side — the body of a TWO-LEVEL GenericBSP walk: bsp_walk (bsp_walk.h) over the top-level tree,
// TransformedPrimitive::Intersect / IntersectP (core/primitive.cpp:77-102) at every leaf primitive that is an object instance, and
// the same walk over the instance's own tree with the transformed ray — what an instanced scene of one of the fork's BSP
// accelerators is in the reference (pbrtObjectInstance, core/api.cpp:1794-1819).  All trees share one node array and one
// primitiveIndices array.  The two-level RBSP walks (rbspinst_walk.hip) and the two-level general BSP walks
// (bsppaperinst_walk.hip) instantiate it; a walk passes its interior step in as `Step`, with bsp_walk's contract:
//   bool leaf(uint32_t flags), uint32_t high(uint32_t flags)   (aboveChild / nPrimitives),
//   void plane(uint32_t flags, float split, vec3 ro, vec3 rd, vec3 invDir, float *tPlane, bool *belowFirst),
// and with KD_SHARE `bool kd(uint32_t flags)` and `void kd_count_add(bool anyHit, uint32_t n)`.  The step keeps no per-ray state
// and is given the ray of the level being walked, so both levels run the same instructions.
// NODE_AXIS (the two-level general BSP walks) gives the step per-node data as bsp_walk's NODE_AXIS does: the step's
// `float4 axis(uint32_t node)` — one entry per node of the SHARED node array, so an object's node finds its object-space axis at
// its own index — is passed to `void plane(float4 axis, uint32_t flags, ...)` in front of the other arguments; requested together
// with the node's 8-byte word (1), or only for the interior nodes for which the step's `bool has_axis(uint32_t flags)` holds (3;
// `plane` gets zeros elsewhere).  0: the step has no per-node data (the RBSP walks), and nothing of this is compiled.
//
// Schedule and todo list are k_kdinstwalk's (kdinst_walk.hip).  One ray per lane; persistent waves draw 64 rays at a time from
// the queue head.  ONE list for both levels: below, the top-level walk's entries {node, tPlane} as in bsp_walk.  Entering an
// instance pushes one entry {top-level leaf node, position of the next primitive in that leaf}: the place the top-level walk
// resumes at when TransformedPrimitive::Intersect returns.  The object's walk pushes above it, from entry `base` on.  A ray
// therefore holds at most depth(top) + 1 + depth(object) entries, which the attach step bounds by the walk's capacity.  The tMax
// stored with an entry is re-read from the tPlane of the entry below it; at the bottom of a level's part of the list there is
// none (for an object the entry below is the saved position, not a tPlane), so each level keeps the root interval's t1 in a
// register: rootTMax and objRootTMax.  The first LDS entries live in LDS ([entry][thread]), the rest in the scene's deep-stack
// area in HBM ([entry][grid thread], DevScene::deepStack).
//
// Counters are the sums over both levels, as r.stats += ray.stats (core/primitive.cpp:84,100) makes them: fetched counts every
// node either walk visits (nbNodeTraversals), entered the interior ones, leaf the leaves; triangle and sphere tests count
// wherever they run; an instance is not itself a primitive test.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "two_level.h"

namespace hprt {

// The whole kernel body.  ANY_HIT: IntersectP (no early-out on a closer hit); COUNT: counters and per-ray statistics; QUAD: the
// scene has spheres.  nodes / primIdx: the attached trees (one-primitive leaves and primIdx hold ORDERED indices over all
// aggregates); entries: two float4 per instance, {lo, root} {hi, prim} (DevInstEntry, two_level.h); lo / hi: the top-level tree's bounds.
// stackMem: the kernel's [LDS][BLOCK] LDS todo entries.
template <bool ANY_HIT, bool COUNT, bool QUAD, int LDS, int BLOCK, class Step, bool KD_SHARE = false, int NODE_AXIS = 0>
__device__ __forceinline__ void bspinst_walk(const DevScene &sc, const uint2 *nodes, const uint32_t *primIdx, const float4 *entries, const float *lo,
                                             const float *hi, Step &step, const uint32_t *queue, const uint32_t *countPtr, uint32_t countImm,
                                             const RayStream &rays, const HitStream &hits, uint8_t *occ, DevCounters *counters, uint4 *rayStats,
                                             uint32_t *workCounter, uint2 *stackMem) {
    uint2 *const ldsStack = &stackMem[threadIdx.x];
    auto deepSlot = [&](int entry) -> volatile uint2 * {
        return (volatile uint2 *)sc.deepStack + (size_t)(entry - LDS) * HPRT_DEEP_THREADS + (blockIdx.x * BLOCK + threadIdx.x);
    };
    auto readEntry = [&](int entry) -> uint2 {
        if (entry < LDS) return ldsStack[entry * BLOCK];
        const volatile uint2 *p = deepSlot(entry);
        return make_uint2(p->x, p->y);
    };
    auto writeEntry = [&](int entry, uint2 e) {
        if (entry < LDS) ldsStack[entry * BLOCK] = e;
        else { volatile uint2 *p = deepSlot(entry); p->x = e.x; p->y = e.y; }
    };
    const uint32_t n = countPtr ? *countPtr : countImm;
    const uint32_t lane = __lane_id();
    TraceCount cnt = {0u, 0u, 0u, 0u, 0u};     // fetched: nbNodeTraversals, entered: interior nodes, leaf: leaves — both levels
    uint32_t kdCnt = 0u;                       // KD_SHARE: of the entered interior nodes, kd ones — both levels
    while (true) {
        uint32_t base0 = 0u;
        if (lane == 0) base0 = atomicAdd(workCounter, 64u);
        base0 = __shfl(base0, 0);
        if (base0 >= n) break;
        const uint32_t idx = base0 + lane;
        if (idx >= n) continue;
        const uint32_t slot = queue ? queue[idx] : idx;
        const float4 ra = rays.a[slot], rb = rays.b[slot];
        vec3 ro(ra.x, ra.y, ra.z), rd(rb.x, rb.y, rb.z);      // the ray of the level being walked: the world ray, or the instance's
        float rayTMax = ra.w;
        const TraceCount snap = cnt;
        const uint32_t kdSnap = kdCnt;
        bool hit = false;
        int32_t prim = -1, hitInst = -1; float hb0 = 0.f, hb1 = 0.f, hb2 = 0.f;
        float tMin, tMax;
        if (inst_root_interval(vec3(lo[0], lo[1], lo[2]), vec3(hi[0], hi[1], hi[2]), ro, rd, rayTMax, &tMin, &tMax)) {
            vec3 invDir(1 / rd.x, 1 / rd.y, 1 / rd.z);
            RayShear shear = ray_shear(rd, invDir);
            const float rootTMax = tMax;
            float objRootTMax = 0.f;          // the root interval's t1 of the instance being walked
            float savedTMax = 0.f;            // the world ray's tMax when the instance was entered
            int sp = 0, base = 0;             // base: first entry of the level being walked (0, or one past the saved position)
            int inst = -1;                    // instance being walked
            bool instHit = false;             // a hit was recorded inside it
            bool direct = false;              // `node` is taken up where it was left (or is a lone primitive's leaf): no tMin test, no node counted
            bool leave = false;               // the instance's walk is over
            uint32_t i0 = 0u;                 // first position to test in the next leaf: nonzero only when a top-level leaf is resumed
            uint32_t node = 0u;
            bool done = false;
            while (!done) {
                if (leave) {
                    // TransformedPrimitive::Intersect returns: r.tMax = ray.tMax only if the instance was hit (core/primitive.cpp:85-86);
                    // back to the world ray (re-read from the stream and re-derived: cheaper than holding it across the object's walk)
                    // and to the next primitive of the top-level leaf the instance sits in
                    leave = false;
                    sp = base - 1;
                    const uint2 e = readEntry(sp);
                    node = e.x; i0 = e.y;
                    base = 0; inst = -1; direct = true;
                    const float4 wa = rays.a[slot], wb = rays.b[slot];
                    ro = vec3(wa.x, wa.y, wa.z); rd = vec3(wb.x, wb.y, wb.z);
                    invDir = vec3(1 / rd.x, 1 / rd.y, 1 / rd.z);
                    shear = ray_shear(rd, invDir);
                    if (!instHit) rayTMax = savedTMax;
                }
                if (!direct) {
                    if (!ANY_HIT && rayTMax < tMin) {      // a hit closer than the current node: this level's walk is over
                        if (inst >= 0) { leave = true; continue; }
                        break;
                    }
                    if (COUNT) ++cnt.fetched;
                }
                uint2 nd = nodes[node];
                [[maybe_unused]] float4 axis;
                if constexpr (NODE_AXIS == 1) {
                    axis = step.axis(node);
                    // an empty asm that takes the node word and the whole entry: both requests are issued before one wait, the
                    // entry as one 16-byte load (bsp_walk.h)
                    asm volatile("" : "+v"(nd.x), "+v"(nd.y), "+v"(axis.x), "+v"(axis.y), "+v"(axis.z), "+v"(axis.w));
                }
                if (!step.leaf(nd.y)) {
                    if (COUNT) ++cnt.entered;
                    if constexpr (COUNT && KD_SHARE) kdCnt += step.kd(nd.y) ? 1u : 0u;
                    float tPlane; bool belowFirst;
                    if constexpr (NODE_AXIS == 3) { axis = make_float4(0.f, 0.f, 0.f, 0.f); if (step.has_axis(nd.y)) axis = step.axis(node); }
                    if constexpr (NODE_AXIS != 0) step.plane(axis, nd.y, __uint_as_float(nd.x), ro, rd, invDir, &tPlane, &belowFirst);
                    else step.plane(nd.y, __uint_as_float(nd.x), ro, rd, invDir, &tPlane, &belowFirst);
                    const uint32_t above = step.high(nd.y);
                    const uint32_t first = belowFirst ? node + 1u : above, second = belowFirst ? above : node + 1u;
                    if (tPlane > tMax || tPlane <= 0) node = first;
                    else if (tPlane < tMin) node = second;
                    else {
                        writeEntry(sp, make_uint2(second, __float_as_uint(tPlane)));
                        ++sp;
                        node = first;
                        tMax = tPlane;
                    }
                } else {
                    if (COUNT && !direct) ++cnt.leaf;
                    direct = false;
                    const uint32_t np = step.high(nd.y);
                    bool entered = false;
                    for (uint32_t i = i0; i < np; ++i) {
                        const uint32_t pi = np == 1u ? nd.x : primIdx[nd.x + i];
                        const float4 v0 = sc.tris[3 * pi], v1 = sc.tris[3 * pi + 1], v2 = sc.tris[3 * pi + 2];
                        const uint32_t tag = __float_as_uint(v0.w);
                        if ((tag & TAG_KIND_MASK) == 0u) {
                            if (COUNT) ++cnt.tri;
                            float b0, b1, b2, t;
                            if (tri_test(vec3(v0.x, v0.y, v0.z), vec3(v1.x, v1.y, v1.z), vec3(v2.x, v2.y, v2.z), ro, rayTMax, shear, &b0, &b1, &b2, &t)) {
                                if (ANY_HIT) { hit = true; done = true; break; }
                                // a zero-area triangle reports no hit to Intersect (shapes/triangle.cpp:309-316), IntersectP does
                                if (!(tag & TAG_BOGUS)) {
                                    hit = true; rayTMax = t; prim = (int32_t)(pi | ((tag & TAG_BIN_MASK) << 24)); hb0 = b0; hb1 = b1; hb2 = b2;
                                    hitInst = inst; instHit = inst >= 0;
                                }
                            }
                        } else if ((tag & TAG_KIND_MASK) == TAG_INSTANCE) {
                            if (inst >= 0) continue;      // (objects hold no instances: core/api.cpp:1785 refuses them)
                            // TransformedPrimitive::Intersect: Ray ray = Inverse(InterpolatedPrimToWorld)(r), i.e.
                            // Transform::operator()(const Ray &) (core/transform.h:251-264); then the wrapped primitive
                            inst = (int)__float_as_uint(v2.w);
                            mat4 W;
                            if (tag & TAG_INST_INLINE) {      // affine: the matrix came with the primitive, its translation sits in topEntry
                                const float4 te = sc.topEntry[pi];
                                W.m[0][0] = v0.x; W.m[0][1] = v0.y; W.m[0][2] = v0.z; W.m[0][3] = te.x;
                                W.m[1][0] = v1.x; W.m[1][1] = v1.y; W.m[1][2] = v1.z; W.m[1][3] = te.y;
                                W.m[2][0] = v2.x; W.m[2][1] = v2.y; W.m[2][2] = v2.z; W.m[2][3] = te.z;
                                W.m[3][0] = 0.f; W.m[3][1] = 0.f; W.m[3][2] = 0.f; W.m[3][3] = 1.f;
                            } else W = sc.instances[inst].w2i;
                            const float4 e0 = entries[2 * inst], e1 = entries[2 * inst + 1];      // {lo, root} {hi, prim}
                            vec3 oErr;
                            vec3 o2 = xf_point_err(W, ro, &oErr);
                            const vec3 d2 = xf_vector(W, rd);
                            const float lengthSquared = d2.x * d2.x + d2.y * d2.y + d2.z * d2.z;
                            float tm = rayTMax;
                            if (lengthSquared > 0) {
                                const float dt = dot(vabs(d2), oErr) / lengthSquared;
                                o2 = o2 + d2 * dt;
                                tm -= dt;
                            }
                            // the top-level walk resumes at the next primitive of this leaf
                            writeEntry(sp, make_uint2(node, i + 1u));
                            ++sp;
                            base = sp;
                            savedTMax = rayTMax; instHit = false;
                            ro = o2; rd = d2; rayTMax = tm;
                            invDir = vec3(1 / d2.x, 1 / d2.y, 1 / d2.z);
                            shear = ray_shear(d2, invDir);
                            node = __float_as_uint(e0.w);
                            if (__float_as_int(e1.w) >= 0) direct = true;      // a lone primitive, wrapped as it is: no bounds test, no node
                            else if (inst_root_interval(vec3(e0.x, e0.y, e0.z), vec3(e1.x, e1.y, e1.z), ro, rd, rayTMax, &tMin, &tMax)) objRootTMax = tMax;
                            else leave = true;                                  // the ray misses the object's bounds
                            entered = true;
                            break;
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
                                hitInst = inst; instHit = inst >= 0;
                            }
                        }
                    }
                    i0 = 0u;
                    if (done) break;
                    if (entered) continue;
                    if (sp == base) {                 // nothing left on this level
                        if (inst >= 0) { leave = true; continue; }
                        break;
                    }
                    --sp;
                    const uint2 e = readEntry(sp);
                    node = e.x;
                    tMin = __uint_as_float(e.y);
                    tMax = sp > base ? __uint_as_float(readEntry(sp - 1).y) : (inst >= 0 ? objRootTMax : rootTMax);
                }
            }
        }
        if (COUNT && rayStats) rayStats[slot] = make_uint4(cnt.entered - snap.entered, cnt.leaf - snap.leaf, (cnt.tri + cnt.sphere) - (snap.tri + snap.sphere),
                                                    KD_SHARE ? kdCnt - kdSnap : 0u);
        if (ANY_HIT) occ[slot] = hit ? 1 : 0;
        else {
            hit_store(hits, slot, hit ? prim : -1, hb0, hb1, hb2, rayTMax, hit ? hitInst : -1);
        }
    }
    if (COUNT) wave_count_add(counters, ANY_HIT, cnt);
    if constexpr (COUNT && KD_SHARE) step.kd_count_add(ANY_HIT, kdCnt);
}

}  // namespace hprt
