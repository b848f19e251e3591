// hprt device side — the two-level kd-tree walk (gfx950, wave64): KdTreeAccel::Intersect / IntersectP
// (accelerators/kdtreeaccel.cpp:381-521) over the top-level tree, TransformedPrimitive::Intersect / IntersectP
// (core/primitive.cpp:77-102) at every leaf primitive that is an object instance, and the same KdTreeAccel walk over the
// instance's own tree with the transformed ray — what an instanced Accelerator "kdtree" scene is in the reference
// (pbrtObjectInstance, core/api.cpp:1794-1819).  All trees share one node array and one primitiveIndices array (kdinst_walk.h,
// DevKdInst).
//
// One ray per lane; persistent waves draw 64 rays at a time from the queue head (one atomic per wave and draw), exactly like
// k_kdwalk (kd_walk.hip): the render loop does not know which walk ran.  The interior step and the leaf loop are k_kdwalk's,
// written once and run by both levels — a lane inside an instance and a lane on the top level execute the same instructions.
//
// Todo list: ONE list for both levels.  Below, the top-level walk's entries {node, tPlane} as in k_kdwalk.  Entering an instance
// pushes one entry {top-level leaf node, position of the next primitive in that leaf}: the place the top-level walk resumes at
// when TransformedPrimitive::Intersect returns.  The object's walk pushes above it, from entry `base` on.  A ray therefore holds
// at most depth(top) + 1 + depth(object) entries, which the attach step bounds by KD_TODO_MAX.  As in k_kdwalk the tMax stored
// with an entry is re-read from the tPlane of the entry below it; at the bottom of a level's part of the list there is none (for
// an object the entry below is the saved position, not a tPlane), so each level keeps the root interval's t1 in a register:
// rootTMax and objRootTMax.  The first HPRT_KDINST_LDS entries live in LDS ([entry][thread]), the rest in the scene's
// deep-stack area in HBM ([entry][grid thread], DevScene::deepStack).
//
// Counters are the sums over both levels, as r.stats += ray.stats (core/primitive.cpp:84,100) makes them: fetched counts every
// node either walk visits (nbNodeTraversals), entered the interior ones, leaf the leaves; triangle and sphere tests count
// wherever they run; an instance is not itself a primitive test.
//
// Built with -ffp-contract=off: every float operation is one IEEE rounding in the reference's order.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include "kdinst_walk.h"
#include "../kdtree_builder.h"

#ifndef HPRT_KDINST_LDS
#define HPRT_KDINST_LDS 8
#endif
#define HPRT_KDINST_BLOCK 256
// workgroups per CU (= waves per SIMD): four for the triangle-only kernels — the two-level state (the instance's ray next to the
// positions of both levels) needs more than the 80 registers six waves leave — and three with the quadric code, whose
// interval-arithmetic call would otherwise push some of that state into scratch
#ifndef HPRT_KDINST_WAVES
#define HPRT_KDINST_WAVES 4
#endif
#define HPRT_KDINST_QUAD_WAVES 3

namespace hprt {

static_assert(HPRT_KDINST_LDS + HPRT_SPILL_STACK >= (int)KD_TODO_MAX, "LDS + deep-stack entries must hold the deepest pair of trees attach accepts");
static_assert(HPRT_DEEP_THREADS >= 256u * HPRT_KDINST_BLOCK * HPRT_KDINST_WAVES && HPRT_DEEP_THREADS >= 256u * HPRT_KDINST_BLOCK * HPRT_KDINST_QUAD_WAVES,
              "the deep-stack area must cover the two-level kd walk's grids");

// ANY_HIT: IntersectP; COUNT: counters and per-ray statistics; QUAD: the scene has spheres (the interval-arithmetic test is
// compiled in only then).
template <bool ANY_HIT, bool COUNT, bool QUAD>
__global__ __launch_bounds__(HPRT_KDINST_BLOCK, QUAD ? HPRT_KDINST_QUAD_WAVES : HPRT_KDINST_WAVES) void k_kdinstwalk(DevScene sc, DevKdInst kd, const uint32_t *queue, const uint32_t *countPtr,
                                                                                    uint32_t countImm, RayStream rays, HitStream hits, uint8_t *occ,
                                                                                    DevCounters *counters, uint4 *rayStats, uint32_t *workCounter) {
    __shared__ uint2 stackMem[HPRT_KDINST_LDS * HPRT_KDINST_BLOCK];     // [entry][thread]: {node, tPlane} or {leaf node, position}
    uint2 *const ldsStack = &stackMem[threadIdx.x];
    auto deepSlot = [&](int entry) -> volatile uint2 * {
        return (volatile uint2 *)sc.deepStack + (size_t)(entry - HPRT_KDINST_LDS) * HPRT_DEEP_THREADS + (blockIdx.x * HPRT_KDINST_BLOCK + threadIdx.x);
    };
    auto readEntry = [&](int entry) -> uint2 {
        if (entry < HPRT_KDINST_LDS) return ldsStack[entry * HPRT_KDINST_BLOCK];
        const volatile uint2 *p = deepSlot(entry);
        return make_uint2(p->x, p->y);
    };
    auto writeEntry = [&](int entry, uint2 e) {
        if (entry < HPRT_KDINST_LDS) ldsStack[entry * HPRT_KDINST_BLOCK] = e;
        else { volatile uint2 *p = deepSlot(entry); p->x = e.x; p->y = e.y; }
    };
    const uint32_t n = countPtr ? *countPtr : countImm;
    const uint32_t lane = __lane_id();
    TraceCount cnt = {0u, 0u, 0u, 0u, 0u};     // fetched: nbNodeTraversals, entered: kdTreeNodeTraversals (interior), leaf: leaves — both levels
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
        bool hit = false;
        int32_t prim = -1, hitInst = -1; float hb0 = 0.f, hb1 = 0.f, hb2 = 0.f;
        float tMin, tMax;
        if (inst_root_interval(vec3(kd.lo[0], kd.lo[1], kd.lo[2]), vec3(kd.hi[0], kd.hi[1], kd.hi[2]), ro, rd, rayTMax, &tMin, &tMax)) {
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
                        writeEntry(sp, make_uint2(second, __float_as_uint(tPlane)));
                        ++sp;
                        node = first;
                        tMax = tPlane;
                    }
                } else {
                    if (COUNT && !direct) ++cnt.leaf;
                    direct = false;
                    const uint32_t np = nd.y >> 2;
                    bool entered = false;
                    for (uint32_t i = i0; i < np; ++i) {
                        const uint32_t pi = np == 1u ? nd.x : kd.primIdx[nd.x + i];
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
                            const float4 *ep = (const float4 *)&kd.entries[inst];
                            const float4 e0 = ep[0], e1 = ep[1];      // {lo, root} {hi, prim}
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
        if (COUNT && rayStats) rayStats[slot] = make_uint4(cnt.entered - snap.entered, cnt.leaf - snap.leaf, (cnt.tri + cnt.sphere) - (snap.tri + snap.sphere), 0u);
        if (ANY_HIT) occ[slot] = hit ? 1 : 0;
        else {
            hit_store(hits, slot, hit ? prim : -1, hb0, hb1, hb2, rayTMax, hit ? hitInst : -1);
        }
    }
    if (COUNT) wave_count_add(counters, ANY_HIT, cnt);
}

void LaunchKdInstTrace(hipStream_t st, const DevScene &sc, const DevKdInst &kd, bool anyHit, bool count, const uint32_t *queue,
                       const uint32_t *countPtr, uint32_t countImm, uint32_t gridItems, const RayStream &rays, const HitStream &hits,
                       uint8_t *occ, DevCounters *counters, uint32_t *workCounter, uint4 *rayStats) {
    LaunchTreeWalk<HPRT_KDINST_BLOCK, HPRT_KDINST_WAVES, HPRT_KDINST_QUAD_WAVES>(st, sc, anyHit, count, gridItems, workCounter, [&](dim3 grid, dim3 block, auto a, auto c, auto q) {
        hipLaunchKernelGGL((k_kdinstwalk<decltype(a)::value, decltype(c)::value, decltype(q)::value>), grid, block, 0, st, sc, kd, queue, countPtr, countImm, rays,
                           hits, occ, counters, rayStats, workCounter);
    });
}

}  // namespace hprt
