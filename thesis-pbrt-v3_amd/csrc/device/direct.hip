// hprt device side — the direct-lighting estimator (gfx950, wave64): DirectLightingIntegrator::Li (integrators/directlighting.cpp:
// 62-100) as four kernels around the scene's own traces.  Li is a TREE per camera sample (SpecularReflect, then SpecularTransmit, each
// a recursive Li: core/integrator.cpp:362-450), walked depth first, one node per camera sample and step; the sampler's dimension and
// array cursors run through the tree in that order (capi_device.hip, RunDlBatch):
//     closest-hit trace                             the step's node rays (step 0: k_generate's camera rays)     the scene's walk
//     k_dl_shade     one lane per node              directlighting.cpp:67-84: Le of escaped rays, the SurfaceInteraction, isect.Le(wo),
//                                                   the sampler cursors past the node's light samples, one record per hit
//     k_dl_rays      one lane per (hit, light, k)   UniformSampleAllLights / UniformSampleOneLight's sample values and EstimateDirect's two
//                                                   halves up to their rays (core/integrator.cpp:55-217)
//     any-hit trace, closest-hit trace              VisibilityTester::Unoccluded; scene.Intersect of the BSDF-sampled rays
//     k_dl_resolve   one lane per hit               the estimates added in the reference's order (per light, k = 0 .. n - 1, light half
//                                                   then BSDF half; no tree reduction: the film is compared bit for bit)
//     k_dl_advance   one lane per node              directlighting.cpp:93-98: the node's SpecularReflect / SpecularTransmit, or — the node
//                                                   is complete — f * Li * AbsDot / pdf into its parent and the parent's next call
// The "!isect.bsdf" retry of directlighting.cpp:76-81 is not built: every material in scope makes a BSDF.  The ray differentials
// SpecularReflect / SpecularTransmit hand their child (core/integrator.cpp:376-393, 416-445) are not built either: they decide texture
// filter widths only, and a scene where a child could meet an image texture is refused (capi_device.hip, CheckDirectScene).
//
// Built with -ffp-contract=off: every float operation below is a single IEEE rounding in the order the reference's scalar code
// performs it.  No inline assembly.
#include <hip/hip_runtime.h>
#include "dev_specular.h"
#include "direct.h"

namespace hprt {

namespace {

// wave-level append: the position for lanes with pred, one atomic per wave
__device__ __forceinline__ uint32_t dl_wave_append(uint32_t *counter, bool pred) {
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

enum : uint32_t { DL_DIM_MASK = 0xffffu, DL_DEPTH_SHIFT = 16u, DL_DEPTH_MASK = 15u, DL_ARRAY_SHIFT = 20u, DL_ARRAY_MASK = 0xffu };
enum : uint32_t { DL_NO_RAY = 0xffffffffu, DL_NO_TERM = 0x40000000u, DL_RAY_MASK = 0x3fffffffu };

__device__ __forceinline__ uint32_t dl_sample_number(const DlSlots &sl, uint32_t slot) { return sl.sampleNum ? sl.sampleNum[slot] : sl.s0 + slot / sl.nPix; }
// GetIndexForSample(sampleNum) of the slot's pixel, 64-bit (samplers/halton.cpp:101-118)
__device__ __forceinline__ uint64_t dl_index(const DlSlots &sl, const DevHalton &hal, uint32_t slot, uint64_t sampleNum) {
    return sl.pixelBase[slot % sl.nPix] + sampleNum * (uint64_t)hal.sampleStride;
}
__device__ __forceinline__ float4 *dl_plane(const DlState &S, uint32_t d, uint32_t k, uint32_t slot) {
    return S.stack + ((size_t)d * DL_STACK_PLANES + k) * S.stride + slot;
}
// the node's SurfaceInteraction as k_dl_shade left it
__device__ __forceinline__ void dl_load_si(const DlState &S, uint32_t d, uint32_t slot, DevSI *si) {
    const float4 p = *dl_plane(S, d, 2, slot), e = *dl_plane(S, d, 3, slot), wo = *dl_plane(S, d, 4, slot), n = *dl_plane(S, d, 5, slot),
                 ns = *dl_plane(S, d, 6, slot), du = *dl_plane(S, d, 7, slot);
    si->p = vec3(p.x, p.y, p.z); si->pErr = vec3(e.x, e.y, e.z); si->wo = vec3(wo.x, wo.y, wo.z); si->n = vec3(n.x, n.y, n.z);
    si->ns = vec3(ns.x, ns.y, ns.z); si->sdpdu = vec3(du.x, du.y, du.z);
    si->shape = 0; si->material = (int32_t)__float_as_uint(e.w);
}

// the radiance guards of core/integrator.cpp:300-321 and the store of sample `slot` (k_store_radiance)
__device__ __forceinline__ void dl_store(const DlRadiance &out, uint32_t slot, rgb L) {
    const float y = luminance(L);
    if (is_nan(L.r) || is_nan(L.g) || is_nan(L.b)) L = rgb(0.f);
    else if ((double)y < -1e-5) L = rgb(0.f);
    else if (is_inf(y)) L = rgb(0.f);
    const size_t o = out.base + slot;
    out.R[o] = L.r; out.G[o] = L.g; out.B[o] = L.b;
}

}  // namespace

// ---------------------------------------------------------------------------
// k_dl_shade: directlighting.cpp:67-84 for the node a live camera sample is at.  An escaped ray's node is complete with the sum of
// every light's Le(ray) (:69-72; zero but for infinite lights, core/light.cpp:66); a hit leaves isect.Le(wo) (:84), its
// SurfaceInteraction (as k_shade's generic variant fills it: triangle or sphere, inside an object instance or not) and a record for
// the light work.  The sampler's cursors move past the node's light samples here, whatever those samples turn out to do:
//     "all", arrays left    Get2DArray twice per light: the array cursor moves on, no dimension is drawn          (core/integrator.cpp:65-66)
//     "all", arrays used up two Get2D per light                                                                   (:69-70)
//     "one"                 Get1D, Get2D, Get2D                                                                   (:99-104)
// TEX: the scene has image textures — evaluated here, at camera-ray hits with the camera's differentials (core/interaction.cpp:103-149).
// ---------------------------------------------------------------------------
template <bool TEX>
__global__ __launch_bounds__(256) void k_dl_shade(DevScene sc, RenderParams rp, DlParams dp, DlSlots sl, RayStream rays, HitStream hit, const uint32_t *live,
                                                  uint32_t nLive, uint32_t first, DlState S, DlRecords recs, uint32_t *hitCount) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool wantRecord = false;
    uint4 q = make_uint4(0u, 0u, 0u, 0u);
    rgb kdTex(0.f), ksTex(0.f), opTex(0.f);
    if (i < nLive) {
        const uint32_t slot = live ? live[i] : i;
        const uint32_t st = first ? (uint32_t)dp.arrayEndDim : S.state[slot];
        uint32_t dim = st & DL_DIM_MASK, arrNode = (st >> DL_ARRAY_SHIFT) & DL_ARRAY_MASK;
        const uint32_t d = (st >> DL_DEPTH_SHIFT) & DL_DEPTH_MASK;
        const float4 hitA = hit_load(hit, i);
        const int32_t prim = hit_prim(hit_word(hitA));
        const float4 rayA = rays.a[i], rayB = rays.b[i];
        const vec3 rayO(rayA.x, rayA.y, rayA.z), rayD(rayB.x, rayB.y, rayB.z);
        if (prim < 0) {
            rgb L(0.f);
            for (uint32_t e = 0; e < sc.nEnvLights; ++e) L = L + env_Le(sc, sc.envLights[e], rayD);
            *dl_plane(S, d, 0, slot) = make_float4(L.r, L.g, L.b, __uint_as_float(2u));
        } else {
            const float4 tv0 = sc.tris[3 * prim], tv1 = sc.tris[3 * prim + 1], tv2 = sc.tris[3 * prim + 2];
            const float2 hitB = hit.b ? hit_load_aux(hit, i) : hit_no_aux();
            DevSI si;
            DevTexGeom tg;
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
                fill_triangle(sc, (uint32_t)prim, tv0, tv1, tv2, hit_b0(hitA), hit_b1(hitA), hit_b2(hitA), r0.d, &si, TEX ? &tg : nullptr);
            else {
                float tt;
                fill_sphere(sc, (int)__float_as_uint(tv1.w), r0, &si, &tt, TEX ? &tg : nullptr);
            }
            if (inst >= 0 && !sc.instances[inst].identity) {      // Transform::operator()(const SurfaceInteraction &), core/transform.cpp:262-297
                const DevInstance &in = sc.instances[inst];
                vec3 pErr;
                si.p = xf_point_err_in(in.i2w, si.p, si.pErr, &pErr); si.pErr = pErr;
                si.n = normalize(xf_normal(in.w2i, si.n));
                si.wo = normalize(xf_vector(in.i2w, si.wo));
                si.ns = normalize(xf_normal(in.w2i, si.ns));
                si.sdpdu = xf_vector(in.i2w, si.sdpdu);
                si.ns = face_forward(si.ns, si.n);
                if (TEX) { tg.dpdu = xf_vector(in.i2w, tg.dpdu); tg.dpdv = xf_vector(in.i2w, tg.dpdv); }
            }
            const int mi = si_material(sc, si);
            // L += isect.Le(wo), directlighting.cpp:84 (SurfaceInteraction::Le, core/interaction.cpp:151-154)
            rgb L(0.f);
            const int al = prim_area_light(sc, prim);
            if (al >= 0) L = L + area_L(sc.lights[al], si.n, si.wo);
            const uint32_t phase = (int32_t)d + 1 < dp.maxDepth ? 0u : 2u;      // "if (depth + 1 < maxDepth)", directlighting.cpp:93
            *dl_plane(S, d, 0, slot) = make_float4(L.r, L.g, L.b, __uint_as_float(phase));
            *dl_plane(S, d, 2, slot) = make_float4(si.p.x, si.p.y, si.p.z, 0.f);
            *dl_plane(S, d, 3, slot) = make_float4(si.pErr.x, si.pErr.y, si.pErr.z, __uint_as_float((uint32_t)mi));
            *dl_plane(S, d, 4, slot) = make_float4(si.wo.x, si.wo.y, si.wo.z, 0.f);
            *dl_plane(S, d, 5, slot) = make_float4(si.n.x, si.n.y, si.n.z, 0.f);
            *dl_plane(S, d, 6, slot) = make_float4(si.ns.x, si.ns.y, si.ns.z, 0.f);
            *dl_plane(S, d, 7, slot) = make_float4(si.sdpdu.x, si.sdpdu.y, si.sdpdu.z, 0.f);
            uint32_t texFlags = 0u;
            if (TEX) {
                const DevMaterial m = sc.materials[mi];
                const int opTexId = m.type == 6 ? m.opTex : -1;
                if (m.KdTex >= 0 || m.KsTex >= 0 || opTexId >= 0) {
                    // SurfaceInteraction::ComputeDifferentials (core/interaction.cpp:103-149): only the camera ray carries differentials
                    DevUvDiff uvd; uvd.dudx = uvd.dvdx = uvd.dudy = uvd.dvdy = 0.f;
                    if (d == 0u) {
                        const uint64_t index = dl_index(sl, rp.hal, slot, dl_sample_number(sl, slot));
                        const float u0 = halton_dim(sc, rp.hal, index, 0), u1 = halton_dim(sc, rp.hal, index, 1);
                        const uint32_t pxy = rp.pixelXY[slot % rp.nPix];
                        const float fx = (float)(int)(pxy & 0xffffu) + u0, fy = (float)(int)(pxy >> 16) + u1;
                        float lu = 0.f, lv = 0.f;
                        if (rp.cam.lensRadius > 0) { lu = halton_dim(sc, rp.hal, index, 3); lv = halton_dim(sc, rp.hal, index, 4); }
                        DevRayDiff rd;
                        camera_ray_diff(rp.cam, fx, fy, lu, lv, &rd);
                        const float s = rp.invSqrtSpp;      // RayDifferential::ScaleDifferentials, core/geometry.h:1222-1227
                        rd.rxO = rayO + (rd.rxO - rayO) * s; rd.ryO = rayO + (rd.ryO - rayO) * s;
                        rd.rxD = rayD + (rd.rxD - rayD) * s; rd.ryD = rayD + (rd.ryD - rayD) * s;
                        compute_differentials(si, tg, rd, &uvd);
                    }
#pragma unroll 1
                    for (int k = 0; k < 3; ++k) {
                        const int id = k == 0 ? m.KdTex : k == 1 ? m.KsTex : opTexId;
                        if (id < 0) continue;
                        const rgb r = eval_image_texture(sc, id, tg, uvd);
                        if (k == 0) kdTex = r; else if (k == 1) ksTex = r; else opTex = r;
                        texFlags |= 1u << k;
                    }
                }
            }
            if (dp.nLights > 0u) {      // "if (scene.lights.size() > 0)", directlighting.cpp:85
                uint32_t mode;
                const uint32_t dimBase = dim, node = arrNode;
                if (dp.strategy == 1) { mode = 2u; dim += 5u; }
                else if ((int32_t)arrNode < dp.maxDepth) { mode = 0u; arrNode += 1u; }      // Get2DArray: array2DOffset < sampleArray2D.size(), core/sampler.cpp:94
                else { mode = 1u; dim += 4u * dp.nLights; }
                q = make_uint4(slot, d | (mode << 8) | (texFlags << 16), dimBase, node);
                wantRecord = true;
            }
        }
        S.state[slot] = dim | (d << DL_DEPTH_SHIFT) | (arrNode << DL_ARRAY_SHIFT);
    }
    const uint32_t pos = dl_wave_append(hitCount, wantRecord);
    if (wantRecord) {
        recs.q[pos] = q;
        if (TEX) {
            recs.tex[pos] = make_float4(kdTex.r, kdTex.g, kdTex.b, 0.f);
            recs.tex[(size_t)recs.stride + pos] = make_float4(ksTex.r, ksTex.g, ksTex.b, 0.f);
            recs.tex[2 * (size_t)recs.stride + pos] = make_float4(opTex.r, opTex.g, opTex.b, 0.f);
        }
    }
}

// ---------------------------------------------------------------------------
// k_dl_rays: work item w = item * nh + hl of the hits [h0, h0 + nh) — consecutive lanes take consecutive hits at the same light and
// sample number, so a wave runs one light's code and reads and writes consecutive words.  The item's two sample values:
//     arrays     element k of the arrays the node drew for light j, 2 * (node * nLights + j) and the next one among the requested
//                arrays (directlighting.cpp:53-58): dimensions 5 + 2 * array and the next at GetIndexForSample(sample * n + k)
//                (core/sampler.cpp:154-164, 93-98) — 64-bit, the global permutation table
//     fallback   Get2D, Get2D at the node's plain dimensions (core/integrator.cpp:69-70)
//     "one"      Get1D picks min((int)(u * nLights), nLights - 1), then Get2D, Get2D (:99-104)
// then EstimateDirect (core/integrator.cpp:109-217; surface interaction, no media, specular = false).
// ---------------------------------------------------------------------------
template <bool TEX>
__global__ __launch_bounds__(256) void k_dl_rays(DevScene sc, RenderParams rp, DlParams dp, DlSlots sl, DlState S, DlRecords recs, uint32_t h0, uint32_t nh,
                                                 uint32_t nWork, DlItems items, DlRays out) {
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    bool wantShadow = false, wantBsdf = false, bsdfTerm = false;
    rgb lightTerm(0.f), scatterTerm(0.f);
    vec3 so, sd, bo, bd;
    uint32_t pickedLight = 0u;
    if (w < nWork) {
        const uint32_t hl = w % nh, item = w / nh, h = h0 + hl;
        const uint4 q = recs.q[h];
        const uint32_t slot = q.x, d = q.y & 0xffu, mode = (q.y >> 8) & 0xffu, texFlags = q.y >> 16, dimBase = q.z, node = q.w;
        const uint32_t sampleNum = dl_sample_number(sl, slot);
        bool active = true;
        uint32_t lightNum = 0u;
        uint64_t index = dl_index(sl, rp.hal, slot, sampleNum);
        int dimL = 0;
        if (mode == 0u) {
            const uint2 il = dp.itemLight[item];
            lightNum = il.x;
            const uint32_t n = (uint32_t)dp.nLightSamples[lightNum];
            index = dl_index(sl, rp.hal, slot, (uint64_t)sampleNum * n + il.y);
            dimL = 5 + 2 * (int)(2u * (node * dp.nLights + lightNum));
        } else if (mode == 1u) {
            active = item < dp.nLights;
            lightNum = item;
            dimL = (int)(dimBase + 4u * item);
        } else {
            active = item == 0u;
            if (active) {
                const int nLights = (int)dp.nLights;
                lightNum = (uint32_t)sel_min((int)(halton_dim(sc, rp.hal, index, (int)dimBase) * nLights), nLights - 1);
            }
            dimL = (int)dimBase + 1;
        }
        pickedLight = lightNum;
        if (active) {
            DevSI si;
            dl_load_si(S, d, slot, &si);
            DevBsdf bsdf;
            rgb kd, ks, op;
            if (TEX && texFlags) {
                const float4 a = recs.tex[h], b = recs.tex[(size_t)recs.stride + h], c = recs.tex[2 * (size_t)recs.stride + h];
                kd = rgb(a.x, a.y, a.z); ks = rgb(b.x, b.y, b.z); op = rgb(c.x, c.y, c.z);
            }
            bsdf_init(sc, si, &bsdf, TEX && (texFlags & 1u) ? &kd : nullptr, TEX && (texFlags & 2u) ? &ks : nullptr, TEX && (texFlags & 4u) ? &op : nullptr);
            const DevLight light = sc.lights[lightNum];
            const bool isDelta = light.type < 2;
            // (point and distant lights read neither value and never reach the BSDF half: lights/point.cpp:44-53, lights/distant.cpp:49-59)
            float ul0 = 0.f, ul1 = 0.f, us0 = 0.f, us1 = 0.f;
            if (!isDelta) {
                ul0 = halton_dim(sc, rp.hal, index, dimL); ul1 = halton_dim(sc, rp.hal, index, dimL + 1);
                us0 = halton_dim(sc, rp.hal, index, dimL + 2); us1 = halton_dim(sc, rp.hal, index, dimL + 3);
            }
            vec3 wi;
            float lightPdf = 0, scatteringPdf = 0;
            DevIt it; it.p = si.p; it.pErr = si.pErr; it.n = si.n;
            DevIt pl;
            const rgb Li = light_sample<true>(sc, light, it, ul0, ul1, &wi, &lightPdf, &pl);
            if (lightPdf > 0 && !is_black(Li)) {
                const rgb f = bsdf_f(bsdf, si.wo, wi) * absdot(wi, si.ns);
                scatteringPdf = bsdf_pdf(bsdf, si.wo, wi);
                if (!is_black(f)) {
                    // Interaction::SpawnRayTo(it), core/interaction.h:73-78: VisibilityTester::Unoccluded (core/light.cpp:59-64)
                    so = offset_ray_origin(it.p, it.pErr, it.n, pl.p - it.p);
                    const vec3 target = offset_ray_origin(pl.p, pl.pErr, pl.n, so - pl.p);
                    sd = target - so;
                    if (isDelta) lightTerm = f * Li / lightPdf;
                    else { const float wt = power_heuristic(lightPdf, scatteringPdf); lightTerm = f * Li * wt / lightPdf; }
                    wantShadow = true;
                }
            }
            if (!isDelta) {
                int sampledType = 0;
                rgb f = bsdf_sample(bsdf, si.wo, &wi, us0, us1, &scatteringPdf, &sampledType);
                f = f * absdot(wi, si.ns);
                if (!is_black(f) && scatteringPdf > 0) {
                    const float lp = light_pdf<true>(sc, light, it, wi);
                    if (lp != 0) {      // "if (lightPdf == 0) return Ld;", core/integrator.cpp:183
                        const float wt = power_heuristic(scatteringPdf, lp);
                        bo = offset_ray_origin(si.p, si.pErr, si.n, wi);
                        bd = wi;
                        // f * Li * Tr * weight / scatteringPdf if the ray reaches the light's emitting side (:191-205; k_dl_resolve looks);
                        // Li: the emitter's L, or light.Le(ray) of an infinite light
                        rgb Lemit(light.I[0], light.I[1], light.I[2]);
                        if (light.type == 4) Lemit = env_Le(sc, sc.envLights[light.shape], wi);
                        bsdfTerm = !is_black(Lemit);      // "if (!Li.IsBlack())", :204
                        scatterTerm = f * Lemit * rgb(1.f) * wt / scatteringPdf;
                        wantBsdf = true;
                    }
                }
            }
        }
    }
    const uint32_t ps = dl_wave_append(out.shadowCount, wantShadow);
    const uint32_t pb = dl_wave_append(out.bsdfCount, wantBsdf);
    if (w < nWork) {
        if (wantShadow) {
            out.shadow.a[ps] = make_float4(so.x, so.y, so.z, 1 - HPRT_SHADOW_EPS);
            out.shadow.b[ps] = make_float4(sd.x, sd.y, sd.z, 0.f);
        }
        if (wantBsdf) {
            out.bsdf.a[pb] = make_float4(bo.x, bo.y, bo.z, HPRT_INF);
            out.bsdf.b[pb] = make_float4(bd.x, bd.y, bd.z, 0.f);
        }
        items.a[w] = make_float4(lightTerm.r, lightTerm.g, lightTerm.b, __uint_as_float(wantShadow ? ps : DL_NO_RAY));
        items.b[w] = make_float4(scatterTerm.r, scatterTerm.g, scatterTerm.b, __uint_as_float(wantBsdf ? (pb | (bsdfTerm ? 0u : DL_NO_TERM)) : DL_NO_RAY));
        items.light[w] = pickedLight;
    }
}

// ---------------------------------------------------------------------------
// k_dl_resolve: one lane per hit.  EstimateDirect's Ld = [unoccluded: light term] + [the BSDF-sampled ray reached the light: its
// term] per item, then
//     arrays     per light j: Ld = sum over k in order; L += Ld / nSamples          (core/integrator.cpp:75-80)
//     fallback   per light j: L += EstimateDirect                                   (:71)
//   and the node's L += that L (directlighting.cpp:88);
//     "one"      the node's L += EstimateDirect / lightPdf, lightPdf = 1 / nLights   (core/integrator.cpp:100, 105-106; directlighting.cpp:91)
// A blocked or black term is skipped, not added as zero.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dl_resolve(DevScene sc, DlParams dp, DlState S, DlRecords recs, uint32_t h0, uint32_t nh, DlItems items, DlRays rays) {
    const uint32_t hl = blockIdx.x * blockDim.x + threadIdx.x;
    if (hl >= nh) return;
    const uint4 q = recs.q[h0 + hl];
    const uint32_t slot = q.x, d = q.y & 0xffu, mode = (q.y >> 8) & 0xffu;
    auto estimate = [&](uint32_t item, uint32_t lightNum) -> rgb {
        rgb Ld(0.f);
        const float4 a = items.a[(size_t)item * nh + hl], b = items.b[(size_t)item * nh + hl];
        const uint32_t ia = __float_as_uint(a.w), ib = __float_as_uint(b.w);
        if (ia != DL_NO_RAY && !rays.occ[ia]) Ld = Ld + rgb(a.x, a.y, a.z);
        if (ib != DL_NO_RAY && !(ib & DL_NO_TERM)) {
            const uint32_t r = ib & DL_RAY_MASK;
            const float4 mh = hit_load(rays.bsdfHit, r);
            const int32_t prim = hit_prim(hit_word(mh));
            const DevLight light = sc.lights[lightNum];
            if (prim < 0) {      // the ray escaped: light.Le(ray), zero but for an infinite light (core/integrator.cpp:201-202)
                if (light.type == 4) Ld = Ld + rgb(b.x, b.y, b.z);
            } else if (light.type != 4 && (!rays.bsdfHit.b || hit_inst(hit_load_aux(rays.bsdfHit, r)) < 0) && prim_area_light(sc, prim) == (int)lightNum) {
                // lightIsect.Le(-wi) (:198-199): the emitter's normal at the hit
                const float4 ma = rays.bsdf.a[r], mb = rays.bsdf.b[r];
                DRay ry; ry.o = vec3(ma.x, ma.y, ma.z); ry.d = vec3(mb.x, mb.y, mb.z); ry.tMax = HPRT_INF;
                DevSI li;
                bool filled;
                if (light.type == 3) { fill_triangle(sc, (uint32_t)prim, hit_b0(mh), hit_b1(mh), hit_b2(mh), ry.d, &li); filled = true; }
                else { float tt; filled = fill_sphere(sc, (int)__float_as_uint(sc.tris[3 * prim + 1].w), ry, &li, &tt); }
                if (filled && (light.twoSided || dot(li.n, -ry.d) > 0)) Ld = Ld + rgb(b.x, b.y, b.z);
            }
        }
        return Ld;
    };
    float4 *const acc = dl_plane(S, d, 0, slot);
    const float4 L4 = *acc;
    rgb L(L4.x, L4.y, L4.z);
    if (mode == 0u) {
        rgb all(0.f);
        for (uint32_t j = 0; j < dp.nLights; ++j) {
            const uint32_t n = (uint32_t)dp.nLightSamples[j], i0 = dp.lightFirstItem[j];
            rgb Ld(0.f);
            for (uint32_t k = 0; k < n; ++k) Ld = Ld + estimate(i0 + k, j);
            all = all + Ld / (float)(int32_t)n;
        }
        L = L + all;
    } else if (mode == 1u) {
        rgb all(0.f);
        for (uint32_t j = 0; j < dp.nLights; ++j) all = all + estimate(j, j);
        L = L + all;
    } else {
        const float lightPdf = 1.f / (float)(int32_t)dp.nLights;      // Float(1) / nLights
        L = L + estimate(0u, items.light[hl]) / lightPdf;
    }
    *acc = make_float4(L.r, L.g, L.b, L4.w);
}

// ---------------------------------------------------------------------------
// k_dl_advance: directlighting.cpp:93-98 and the way back up.  The node a live sample is at has its Le and direct lighting; what
// remains of Li are its two specular calls, each of which draws its Get2D before it tests anything (core/integrator.cpp:369, 410):
//     phase 0   SpecularReflect: a child through a lobe matching BSDF_REFLECTION | BSDF_SPECULAR
//     phase 1   SpecularTransmit: BSDF_TRANSMISSION | BSDF_SPECULAR — after the reflect subtree, whose nodes have moved the cursors
//     phase 2   the node is complete: its parent adds f * Li * AbsDot(wi, ns) / pdf (:394, 446) and goes on with its own next phase
// The loop ends when a child's ray has been queued for the next step, or the camera ray's node is complete: the sample's radiance.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dl_advance(DevScene sc, RenderParams rp, DlParams dp, DlSlots sl, const uint32_t *live, uint32_t nLive, DlState S,
                                                    RayStream next, uint32_t *nextLive, uint32_t *nextCount, DlRadiance out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool wantNext = false;
    uint32_t slot = 0u;
    vec3 ro, rd;
    if (i < nLive) {
        slot = live ? live[i] : i;
        const uint32_t st = S.state[slot];
        uint32_t dim = st & DL_DIM_MASK, d = (st >> DL_DEPTH_SHIFT) & DL_DEPTH_MASK;
        const uint32_t arrNode = (st >> DL_ARRAY_SHIFT) & DL_ARRAY_MASK;
        const uint64_t index = dl_index(sl, rp.hal, slot, dl_sample_number(sl, slot));
        for (;;) {
            float4 *const acc = dl_plane(S, d, 0, slot);
            const float4 L4 = *acc;
            const uint32_t phase = __float_as_uint(L4.w);
            if (phase == 2u) {
                const rgb Li(L4.x, L4.y, L4.z);
                if (d == 0u) { dl_store(out, slot, Li); break; }
                d -= 1u;
                float4 *const pacc = dl_plane(S, d, 0, slot);
                const float4 P4 = *pacc, fw = *dl_plane(S, d, 1, slot);
                const float pdf = dl_plane(S, d, 2, slot)->w;
                const rgb add = rgb(fw.x, fw.y, fw.z) * Li * fw.w / pdf;
                *pacc = make_float4(P4.x + add.r, P4.y + add.g, P4.z + add.b, P4.w);
                continue;
            }
            // (phase < 2 only where depth + 1 < maxDepth: k_dl_shade)
            acc->w = __uint_as_float(phase + 1u);
            const float u0 = halton_dim(sc, rp.hal, index, (int)dim);      // sampler.Get2D(); no specular lobe reads the second value
            dim += 2u;
            DevSI si;
            dl_load_si(S, d, slot, &si);
            DevBsdf bsdf;
            bsdf_init(sc, si, &bsdf);
            vec3 wi;
            float pdf = 0.f;
            const rgb f = bsdf_sample_specular(bsdf, si.wo, &wi, u0, 0.f, &pdf, phase == 0u ? BX_MASK_SPECULAR_REFLECT : BX_MASK_SPECULAR_TRANSMIT);
            if (pdf > 0.f && !is_black(f) && absdot(wi, si.ns) != 0.f) {
                *dl_plane(S, d, 1, slot) = make_float4(f.r, f.g, f.b, absdot(wi, si.ns));
                dl_plane(S, d, 2, slot)->w = pdf;
                ro = offset_ray_origin(si.p, si.pErr, si.n, wi);      // isect.SpawnRay(wi)
                rd = wi;
                d += 1u;
                wantNext = true;
                break;
            }
        }
        S.state[slot] = dim | (d << DL_DEPTH_SHIFT) | (arrNode << DL_ARRAY_SHIFT);
    }
    const uint32_t pos = dl_wave_append(nextCount, wantNext);
    if (wantNext) {
        next.a[pos] = make_float4(ro.x, ro.y, ro.z, HPRT_INF);
        next.b[pos] = make_float4(rd.x, rd.y, rd.z, 0.f);
        nextLive[pos] = slot;
    }
}

static inline uint32_t dl_blocks_for(size_t n, uint32_t bs) { return (uint32_t)((n + bs - 1) / bs); }

void LaunchDlShade(hipStream_t st, const DevScene &sc, const RenderParams &rp, const DlParams &dp, const DlSlots &sl, const RayStream &rays,
                   const HitStream &hit, const uint32_t *live, uint32_t nLive, bool first, const DlState &state, const DlRecords &recs, uint32_t *hitCount) {
    if (!nLive) return;
    if (sc.textures) hipLaunchKernelGGL(k_dl_shade<true>, dim3(dl_blocks_for(nLive, 256)), dim3(256), 0, st, sc, rp, dp, sl, rays, hit, live, nLive, first ? 1u : 0u, state, recs, hitCount);
    else hipLaunchKernelGGL(k_dl_shade<false>, dim3(dl_blocks_for(nLive, 256)), dim3(256), 0, st, sc, rp, dp, sl, rays, hit, live, nLive, first ? 1u : 0u, state, recs, hitCount);
}
void LaunchDlRays(hipStream_t st, const DevScene &sc, const RenderParams &rp, const DlParams &dp, const DlSlots &sl, const DlState &state,
                  const DlRecords &recs, uint32_t h0, uint32_t nh, const DlItems &items, const DlRays &rays) {
    const uint32_t nWork = nh * dp.itemsPerHit;
    if (!nWork) return;
    if (sc.textures) hipLaunchKernelGGL(k_dl_rays<true>, dim3(dl_blocks_for(nWork, 256)), dim3(256), 0, st, sc, rp, dp, sl, state, recs, h0, nh, nWork, items, rays);
    else hipLaunchKernelGGL(k_dl_rays<false>, dim3(dl_blocks_for(nWork, 256)), dim3(256), 0, st, sc, rp, dp, sl, state, recs, h0, nh, nWork, items, rays);
}
void LaunchDlResolve(hipStream_t st, const DevScene &sc, const DlParams &dp, const DlState &state, const DlRecords &recs, uint32_t h0, uint32_t nh,
                     const DlItems &items, const DlRays &rays) {
    if (nh) hipLaunchKernelGGL(k_dl_resolve, dim3(dl_blocks_for(nh, 256)), dim3(256), 0, st, sc, dp, state, recs, h0, nh, items, rays);
}
void LaunchDlAdvance(hipStream_t st, const DevScene &sc, const RenderParams &rp, const DlParams &dp, const DlSlots &sl, const uint32_t *live,
                     uint32_t nLive, const DlState &state, const RayStream &next, uint32_t *nextLive, uint32_t *nextCount, const DlRadiance &out) {
    if (nLive) hipLaunchKernelGGL(k_dl_advance, dim3(dl_blocks_for(nLive, 256)), dim3(256), 0, st, sc, rp, dp, sl, live, nLive, state, next, nextLive, nextCount, out);
}

}  // namespace hprt
