// hprt device side — BSDF::Sample_f (core/reflection.cpp:703-762) under one of the two lobe masks the reference's
// SamplerIntegrator::SpecularReflect / SpecularTransmit pass (core/integrator.cpp:368, 411): BSDF_REFLECTION | BSDF_SPECULAR and
// BSDF_TRANSMISSION | BSDF_SPECULAR.  BxDF::MatchesFlags ((type & mask) == type, core/reflection.h:219) then lets through
//     mirror          its SpecularReflection(Kr, FresnelNoOp)                                                  (materials/mirror.cpp:44-56)
//     uber            SpecularReflection(op * Kr, FresnelDielectric(1, e)); SpecularTransmission(1 - op, 1, 1) and
//                     SpecularTransmission(op * Kt, 1, e), in that order — the one BSDF that can offer two lobes  (materials/uber.cpp:45-108)
//     smooth glass    SpecularReflection(Kr, FresnelDielectric(1, eta)) and SpecularTransmission(Kt, 1, eta): the lobes
//                     GlassMaterial adds WITHOUT allowMultipleLobes (materials/glass.cpp:62-90), which is how
//                     DirectLightingIntegrator::Li asks for the scattering functions (integrators/directlighting.cpp:75,
//                     core/interaction.h:132).  With allowMultipleLobes — the path integrator's call, and what bsdf_sample(all) restates —
//                     the same material is ONE FresnelSpecular lobe, which is both reflection and transmission and matches neither mask.
// and nothing else: every other lobe in scope is diffuse or glossy.  A header of its own: dev_shading.h is compiled into libhprt.so's
// kernels, this is not.
#pragma once
#include "dev_shading.h"

namespace hprt {

enum : int { BX_MASK_SPECULAR_REFLECT = BX_REFLECTION | BX_SPECULAR, BX_MASK_SPECULAR_TRANSMIT = BX_TRANSMISSION | BX_SPECULAR };

// mask: one of the two above.  *pdf keeps its incoming value on the "wo.z == 0" early return, as in the reference (:729-730; its callers
// leave pdf uninitialised there — ours pass 0).  u1 is drawn and unused: no specular lobe reads its sample.
__device__ __forceinline__ rgb bsdf_sample_specular(const DevBsdf &b, vec3 woW, vec3 *wiW, float u0, float u1, float *pdf, int mask) {
    (void)u1;
    const bool reflect = mask == BX_MASK_SPECULAR_REFLECT;
    // the matching lobes, in the order their material added them: at most one reflection, at most two transmissions
    rgb R(0.f), T0(0.f), T1(0.f);
    bool noOp = false;           // the reflection lobe's Fresnel term is FresnelNoOp (mirror), else FresnelDielectric(1, e)
    float e = 1.f;               // etaB of the reflection lobe's FresnelDielectric and of the second transmission lobe
    if (b.kind == 5) {
        const DevMaterial &m = *b.uber;
        e = m.eta;
        R = b.op * clamp0(rgb(m.Kr[0], m.Kr[1], m.Kr[2]));
        T0 = clamp0(-b.op + rgb(1.f));
        T1 = b.op * clamp0(rgb(m.Kt[0], m.Kt[1], m.Kt[2]));
    } else if (b.kind == 4) { e = b.eta; R = b.Rr; T1 = b.Rd; }
    else if (b.kind == 0 && b.hasR) { noOp = true; R = b.Rr; }
    const int nT0 = is_black(T0) ? 0 : 1, nT1 = is_black(T1) ? 0 : 1;
    const int matching = reflect ? (is_black(R) ? 0 : 1) : nT0 + nT1;
    if (matching == 0) { *pdf = 0; return rgb(0.f); }
    const int comp = sel_min((int)floorf(u0 * matching), matching - 1);
    const vec3 wo = to_local(b, woW);
    if (wo.z == 0) return rgb(0.f);
    *pdf = 0;
    if (reflect) {      // SpecularReflection::Sample_f, core/reflection.cpp:136-143
        const vec3 wi(-wo.x, -wo.y, wo.z);
        *pdf = 1;
        *wiW = to_world(b, wi);
        return (noOp ? rgb(1.f) : rgb(fr_dielectric(cos_theta(wi), 1.f, e))) * R / abs_cos_theta(wi);
    }
    // SpecularTransmission::Sample_f, core/reflection.cpp:145-163 (etaA = 1, TransportMode::Radiance)
    const bool first = nT0 == 1 && comp == 0;
    const rgb T = first ? T0 : T1;
    const float etaB = first ? 1.f : e;
    const bool entering = cos_theta(wo) > 0;
    const float etaI = entering ? 1.f : etaB, etaT = entering ? etaB : 1.f;
    // Refract(wo, Faceforward(Normal3f(0, 0, 1), wo), etaI / etaT, wi), core/reflection.h:96-108
    const vec3 n = face_forward(vec3(0.f, 0.f, 1.f), wo);
    const float er = etaI / etaT;
    const float cosThetaI = dot(n, wo);
    const float sin2ThetaI = sel_max(0.f, 1 - cosThetaI * cosThetaI);
    const float sin2ThetaT = er * er * sin2ThetaI;
    if (sin2ThetaT >= 1) return rgb(0.f);      // total internal reflection: BSDF::Sample_f sees pdf == 0 (:737-740)
    const float cosThetaT = sqrtf(1 - sin2ThetaT);
    const vec3 wi = er * -wo + (er * cosThetaI - cosThetaT) * n;
    rgb ft = T * (rgb(1.f) - rgb(fr_dielectric(cos_theta(wi), 1.f, etaB)));
    ft = ft * ((etaI * etaI) / (etaT * etaT));
    *pdf = 1;
    *wiW = to_world(b, wi);
    if (matching > 1) *pdf /= matching;      // (:748; specular lobes add no pdf of their own, :744-747)
    return ft / abs_cos_theta(wi);
}

// the material's BSDF can offer a lobe to one of the two masks (what decides whether the recursion can leave a surface)
__device__ __forceinline__ bool bsdf_has_specular_lobe(const DevBsdf &b) {
    if (b.kind == 4) return true;
    if (b.kind == 0) return b.hasR;
    if (b.kind != 5) return false;
    const DevMaterial &m = *b.uber;
    return !is_black(clamp0(-b.op + rgb(1.f))) || !is_black(b.op * clamp0(rgb(m.Kr[0], m.Kr[1], m.Kr[2]))) ||
           !is_black(b.op * clamp0(rgb(m.Kt[0], m.Kt[1], m.Kt[2])));
}

}  // namespace hprt
