// hprt device side — the ambient-occlusion estimator (gfx950, wave64): AOIntegrator::Li (integrators/ao.cpp:57-103) as three
// kernels around the scene's own traces.  Per batch of camera samples (capi_device.hip, RunAoBatch):
//     k_generate, closest-hit trace      the camera rays                       unchanged (kernels.hip, the scene's walk)
//     k_ao_frame     one lane per camera sample    the hit's SurfaceInteraction and frame (ao.cpp:67-79), one record per hit
//     k_ao_rays      one lane per hemisphere ray   the array sample, wi, the spawned ray and its term (ao.cpp:81-99)
//     any-hit trace                                 Scene::IntersectP of those rays (the scene's walk, never the shadow grid)
//     k_ao_resolve   one lane per hit              L += term of the unoccluded rays, in sample order (ao.cpp:98-99)
// The "!isect.bsdf" retry of ao.cpp:69-73 is not built: every material in scope makes a BSDF and there are no media, so
// ComputeScatteringFunctions never leaves isect.bsdf null.  The rays carry no time: no transform in scope is animated.
//
// Built with -ffp-contract=off: every float operation below is a single IEEE rounding in the order the reference's scalar code
// performs it.
#include <hip/hip_runtime.h>
#include "dev_shading.h"
#include "ao.h"

namespace hprt {

namespace {

__device__ __forceinline__ uint32_t ao_min(uint32_t a, uint32_t b) { return b < a ? b : a; }
// wave-level append: the position for lanes with pred, one atomic per wave
__device__ __forceinline__ uint32_t ao_wave_append(uint32_t *counter, bool pred) {
    const unsigned long long mask = __ballot(pred);
    if (mask == 0ull) return 0u;
    const uint32_t lane = __lane_id();
    const uint32_t prefix = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
    const int leader = __ffsll((long long)mask) - 1;
    uint32_t base = 0u;
    if ((int)lane == leader) base = atomicAdd(counter, (uint32_t)__popcll(mask));
    base = __shfl(base, leader);
    return base + prefix;
}

// the radiance guards of core/integrator.cpp:300-321 on L = Spectrum(v), and the store of sample `slot` (k_store_radiance)
__device__ __forceinline__ void ao_store(const AoRadiance &out, uint32_t slot, float v) {
    rgb L(v, v, v);
    const float y = luminance(L);
    if (is_nan(L.r) || is_nan(L.g) || is_nan(L.b)) L = rgb(0.f);
    else if ((double)y < -1e-5) L = rgb(0.f);
    else if (is_inf(y)) L = rgb(0.f);
    const size_t o = out.base + slot;
    out.R[o] = L.r; out.G[o] = L.g; out.B[o] = L.b;
}

}  // namespace

// ---------------------------------------------------------------------------
// k_ao_frame: scene.Intersect's SurfaceInteraction (as k_shade's generic variant fills it: triangle or sphere, inside an object
// instance or not) and the frame of ao.cpp:75-79.  A camera ray that escaped stores L = 0 and queues nothing.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ao_frame(DevScene sc, RenderParams rp, RayStream rays, HitStream hit, uint32_t nSlots, uint32_t s0, uint32_t nSamples,
                                                  const uint64_t *aoBase, AoRecords recs, uint32_t *hitCount, AoRadiance out) {
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    bool found = false;
    vec3 p, pErr, n, ss, ts;
    float flipped = 0.f;
    uint64_t index = 0;
    if (slot < nSlots) {
        const float4 hitA = hit_load(hit, slot);
        const int32_t prim = hit_prim(hit_word(hitA));
        found = prim >= 0;
        if (found) {
            const float4 rayA = rays.a[slot], rayB = rays.b[slot];
            const float4 tv0 = sc.tris[3 * prim], tv1 = sc.tris[3 * prim + 1], tv2 = sc.tris[3 * prim + 2];
            const float2 hitB = hit.b ? hit_load_aux(hit, slot) : hit_no_aux();
            const vec3 rayO(rayA.x, rayA.y, rayA.z), rayD(rayB.x, rayB.y, rayB.z);
            DevSI si;
            DevTexGeom tg;      // (dpdu: the geometric one, of which ao.cpp:78 makes s)
            // TransformedPrimitive::Intersect, core/primitive.cpp:77-93: filled in instance space, transformed back
            const int inst = hit_inst(hitB);
            DRay r0; r0.o = rayO; r0.d = rayD; r0.tMax = rayA.w;
            if (inst >= 0) {      // Transform::operator()(const Ray &), core/transform.h:251-264
                const DevInstance &in = sc.instances[inst];
                vec3 oErr;
                r0.o = xf_point_err(in.w2i, rayO, &oErr);
                r0.d = xf_vector(in.w2i, rayD);
                const float lengthSquared = r0.d.x * r0.d.x + r0.d.y * r0.d.y + r0.d.z * r0.d.z;
                if (lengthSquared > 0) {
                    const float dt = dot(vabs(r0.d), oErr) / lengthSquared;
                    r0.o = r0.o + r0.d * dt;
                    r0.tMax -= dt;
                }
            }
            if ((__float_as_uint(tv0.w) & TAG_KIND_MASK) == 0u)
                fill_triangle(sc, (uint32_t)prim, tv0, tv1, tv2, hit_b0(hitA), hit_b1(hitA), hit_b2(hitA), r0.d, &si, &tg);
            else {
                float tt;
                fill_sphere(sc, (int)__float_as_uint(tv1.w), r0, &si, &tt, &tg);
            }
            if (inst >= 0 && !sc.instances[inst].identity) {      // Transform::operator()(const SurfaceInteraction &), core/transform.cpp:262-297
                const DevInstance &in = sc.instances[inst];
                vec3 e;
                si.p = xf_point_err_in(in.i2w, si.p, si.pErr, &e); si.pErr = e;
                si.n = normalize(xf_normal(in.w2i, si.n));
                tg.dpdu = xf_vector(in.i2w, tg.dpdu);
            }
            p = si.p; pErr = si.pErr; n = si.n;
            // ao.cpp:77-79: n faces the camera ray; s and t come from the geometry as it is (t from the UNFLIPPED isect.n)
            flipped = dot(si.n, -rayD) < 0.f ? 1.f : 0.f;      // Faceforward(isect.n, -ray.d), geometry.h:1326-1329
            ss = normalize(tg.dpdu);
            ts = cross(si.n, ss);
            // GetIndexForSample(s * nSamples) of the pixel's sample s: its first array sample (core/sampler.cpp:93-98, 154-164)
            if (aoBase) index = aoBase[slot];
            else {
                const uint32_t pix = slot % rp.nPix, sIdx = slot / rp.nPix;
                index = (uint64_t)rp.pixelOffset[pix] + (uint64_t)(s0 + sIdx) * (uint64_t)nSamples * (uint64_t)rp.hal.sampleStride;
            }
        } else
            ao_store(out, slot, 0.f);
    }
    const uint32_t pos = ao_wave_append(hitCount, found);
    if (found) {
        float4 *r = recs.rec + pos;
        r[0] = make_float4(p.x, p.y, p.z, __uint_as_float(slot));
        r[recs.stride] = make_float4(pErr.x, pErr.y, pErr.z, 0.f);
        r[2 * (size_t)recs.stride] = make_float4(n.x, n.y, n.z, flipped);
        r[3 * (size_t)recs.stride] = make_float4(ss.x, ss.y, ss.z, __uint_as_float((uint32_t)index));
        r[4 * (size_t)recs.stride] = make_float4(ts.x, ts.y, ts.z, __uint_as_float((uint32_t)(index >> 32)));
    }
}

// ---------------------------------------------------------------------------
// k_ao_rays: ao.cpp:81-98 for ray r = hit * nSamples + i.  The lanes of a workgroup cover at most 256 consecutive hits, whose
// records are staged in LDS by consecutive lanes: every record is read from HBM once per workgroup, not once per ray.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ao_rays(DevScene sc, DevHalton hal, AoRecords recs, uint32_t h0, uint32_t nRays, uint32_t nSamples, uint32_t cosSample,
                                                 RayStream out, float *term) {
    __shared__ float4 lds[AO_RECORD_PLANES][256];
    const uint32_t first = blockIdx.x * 256u, last = ao_min(first + 255u, nRays - 1u);      // (the grid has no workgroup beyond nRays)
    const uint32_t hA = first / nSamples, hB = last / nSamples;                                // hits of this workgroup, relative to h0
    if (threadIdx.x <= hB - hA)
        for (uint32_t k = 0; k < AO_RECORD_PLANES; ++k) lds[k][threadIdx.x] = recs.rec[(size_t)k * recs.stride + h0 + hA + threadIdx.x];
    __syncthreads();
    const uint32_t r = first + threadIdx.x;
    if (r >= nRays) return;
    const uint32_t h = r / nSamples, i = r - h * nSamples, l = h - hA;
    const float4 r0 = lds[0][l], r1 = lds[1][l], r2 = lds[2][l], r3 = lds[3][l], r4 = lds[4][l];
    const vec3 p(r0.x, r0.y, r0.z), pErr(r1.x, r1.y, r1.z), ng(r2.x, r2.y, r2.z), s(r3.x, r3.y, r3.z), t(r4.x, r4.y, r4.z);
    const vec3 n = r2.w != 0.f ? -ng : ng;      // Faceforward(isect.n, -ray.d)
    // u[i] of Get2DArray: dimensions arrayStartDim = 5 and 6 at GetIndexForSample(s * nSamples + i), 64-bit
    const uint64_t index = ((uint64_t)__float_as_uint(r3.w) | ((uint64_t)__float_as_uint(r4.w) << 32)) + (uint64_t)i * (uint64_t)hal.sampleStride;
    const float u0 = halton_dim(sc, hal, index, 5), u1 = halton_dim(sc, hal, index, 6);
    vec3 wi;
    float pdf;
    if (cosSample) {      // CosineSampleHemisphere (core/sampling.h:159-163), CosineHemispherePdf(|wi.z|) (:165)
        float dx, dy; concentric_disk(u0, u1, &dx, &dy);
        const float z = sqrtf(sel_max(0.f, 1 - dx * dx - dy * dy));
        wi = vec3(dx, dy, z);
        pdf = fabsf(wi.z) * HPRT_INV_PI;
    } else {              // UniformSampleHemisphere (core/sampling.cpp:89-94), UniformHemispherePdf (:96)
        const float z = u0;
        const float rr = sqrtf(sel_max(0.f, 1.f - z * z));
        const float phi = 2 * HPRT_PI * u1;
        float sn, cs; det_sincosf(phi, &sn, &cs);
        wi = vec3(rr * cs, rr * sn, z);
        pdf = HPRT_INV_2PI;
    }
    // ao.cpp:94-96: to world space, three-term sums in this order
    wi = vec3(s.x * wi.x + t.x * wi.y + n.x * wi.z, s.y * wi.x + t.y * wi.y + n.y * wi.z, s.z * wi.x + t.z * wi.y + n.z * wi.z);
    // isect.SpawnRay(wi), core/interaction.h:73-76: OffsetRayOrigin over the interaction's own n, tMax = Infinity
    const vec3 o = offset_ray_origin(p, pErr, ng, wi);
    out.a[r] = make_float4(o.x, o.y, o.z, HPRT_INF);
    out.b[r] = make_float4(wi.x, wi.y, wi.z, 0.f);
    // Dot(wi, n) / (pdf * nSamples), ao.cpp:99 (pdf * nSamples formed in float first)
    term[r] = dot(wi, n) / (pdf * (float)(int32_t)nSamples);
}

// ---------------------------------------------------------------------------
// k_ao_resolve: L = 0, then L += term for every ray that IntersectP did not stop, i = 0 .. nSamples - 1 in that order (ao.cpp:82-99: no
// tree reduction, the film is compared bit for bit).  One wave per 64 hits: their 64 * nSamples terms and bytes are consecutive, so
// they are read 64 columns at a time by rows (consecutive lanes, consecutive addresses) into LDS and summed by columns.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_ao_resolve(AoRecords recs, uint32_t h0, uint32_t nHits, uint32_t nSamples, const uint8_t *occ, const float *term,
                                                   AoRadiance out) {
    __shared__ float tTile[64][65];
    __shared__ uint8_t oTile[64][68];
    const uint32_t lane = threadIdx.x, hFirst = blockIdx.x * 64u;
    const uint32_t rows = ao_min(64u, nHits - hFirst);      // (the grid has no workgroup beyond nHits)
    float L = 0.f;
    for (uint32_t i0 = 0; i0 < nSamples; i0 += 64u) {
        const uint32_t cols = ao_min(64u, nSamples - i0);
        if (i0) __syncthreads();
        if (lane < cols)
            for (uint32_t row = 0; row < rows; ++row) {
                const size_t r = (size_t)(hFirst + row) * nSamples + i0 + lane;
                tTile[row][lane] = term[r]; oTile[row][lane] = occ[r];
            }
        __syncthreads();
        if (lane < rows)
            for (uint32_t c = 0; c < cols; ++c)
                if (!oTile[lane][c]) L += tTile[lane][c];
    }
    if (lane < rows) ao_store(out, __float_as_uint(recs.rec[h0 + hFirst + lane].w), L);
}

static inline uint32_t ao_blocks_for(size_t n, uint32_t bs) { return (uint32_t)((n + bs - 1) / bs); }

void LaunchAoFrame(hipStream_t st, const DevScene &sc, const RenderParams &rp, const RayStream &rays, const HitStream &hit, uint32_t nSlots, uint32_t s0,
                   uint32_t nSamples, const uint64_t *aoBase, const AoRecords &recs, uint32_t *hitCount, const AoRadiance &out) {
    if (nSlots) hipLaunchKernelGGL(k_ao_frame, dim3(ao_blocks_for(nSlots, 256)), dim3(256), 0, st, sc, rp, rays, hit, nSlots, s0, nSamples, aoBase, recs, hitCount, out);
}
void LaunchAoRays(hipStream_t st, const DevScene &sc, const DevHalton &hal, const AoRecords &recs, uint32_t h0, uint32_t nHits, uint32_t nSamples,
                  bool cosSample, const RayStream &out, float *term) {
    const uint32_t nRays = nHits * nSamples;
    if (nRays) hipLaunchKernelGGL(k_ao_rays, dim3(ao_blocks_for(nRays, 256)), dim3(256), 0, st, sc, hal, recs, h0, nRays, nSamples, cosSample ? 1u : 0u, out, term);
}
void LaunchAoResolve(hipStream_t st, const AoRecords &recs, uint32_t h0, uint32_t nHits, uint32_t nSamples, const uint8_t *occ, const float *term,
                     const AoRadiance &out) {
    if (nHits) hipLaunchKernelGGL(k_ao_resolve, dim3(ao_blocks_for(nHits, 64)), dim3(64), 0, st, recs, h0, nHits, nSamples, occ, term, out);
}

}  // namespace hprt
