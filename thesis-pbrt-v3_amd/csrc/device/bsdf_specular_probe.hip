// hprt — k_bsdf_specular_probe: bsdf_sample_specular (dev_specular.h), the BSDF::Sample_f of SpecularReflect / SpecularTransmit
// (core/integrator.cpp:362-450), evaluated on gfx950 over host arrays of (shape, frame, wo, u) queries under either lobe mask, so that
// a test can hold it against the oracle's lobe-array BSDF::Sample_f directly: every material, both masks, both sides of the uber
// lobe choice, grazing directions and wo.z == 0.  No texture overrides: the material's constants.
//
// A translation unit of its own with a pinned CUID (build.py), linked into libhprt_probe.so: libhprt.so gains no code object.
// Diagnostics only; not part of include/hprt.h.
#include <hip/hip_runtime.h>
#include <vector>
#include "../../../include/hprt.h"
#include "../device_state.h"
#include "dev_specular.h"

namespace hprt {
namespace {

// One query per thread.  frame9: n, ns (shading.n), sdpdu (shading.dpdu).  out8: f (3), wiW (3), pdf, 1 if the material can offer either
// mask a lobe — pdf and wiW preset to -7 and (9, 9, 9), so that the early return that leaves them untouched shows
__global__ __launch_bounds__(256) void k_bsdf_specular_probe(DevScene sc, int mask, size_t n, const int32_t *__restrict__ shape, const float *__restrict__ frame9,
                                                              const float *__restrict__ wo3, const float *__restrict__ u2, float *__restrict__ out8) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *fr = frame9 + 9 * i;
    DevSI si;
    si.p = vec3(0.f, 0.f, 0.f); si.pErr = vec3(0.f, 0.f, 0.f); si.wo = vec3(0.f, 0.f, 0.f);      // (unused by the BSDF)
    si.n = vec3(fr[0], fr[1], fr[2]); si.ns = vec3(fr[3], fr[4], fr[5]); si.sdpdu = vec3(fr[6], fr[7], fr[8]);
    si.shape = shape[i]; si.material = -1;
    DevBsdf b;
    bsdf_init(sc, si, &b);
    const vec3 wo(wo3[3 * i], wo3[3 * i + 1], wo3[3 * i + 2]);
    float pdf = -7.0f; vec3 w(9.f, 9.f, 9.f);
    const rgb f = bsdf_sample_specular(b, wo, &w, u2[2 * i], u2[2 * i + 1], &pdf, mask);
    float4 *dst = (float4 *)(out8 + 8 * i);      // (hipMalloc'ed base, 32 bytes per query)
    dst[0] = make_float4(f.r, f.g, f.b, w.x);
    dst[1] = make_float4(w.y, w.z, pdf, bsdf_has_specular_lobe(b) ? 1.f : 0.f);
}

}  // namespace
}  // namespace hprt

using namespace hprt;

// Diagnostics hook: out8[8 * i ..] = bsdf_sample_specular of shapes[shape[i]]'s material at the frame frame9[9 * i ..] for wo3 / u2 [i]
// under mask (17: BSDF_REFLECTION | BSDF_SPECULAR, 18: BSDF_TRANSMISSION | BSDF_SPECULAR).  Refused without a launch: a null pointer,
// n == 0 or n > 2^22, another mask, a shape index outside the scene's shapes, a material with an image texture on Kd, Ks or opacity.
extern "C" __attribute__((visibility("default"))) int hprt_debug_device_bsdf_specular(HprtScene *s, int mask, size_t n, const int32_t *shape, const float *frame9,
                                                                                        const float *wo3, const float *u2, float *out8) try {
    if (!s || !shape || !frame9 || !wo3 || !u2 || !out8 || n == 0 || n > ((size_t)1 << 22) || (mask != BX_MASK_SPECULAR_REFLECT && mask != BX_MASK_SPECULAR_TRANSMIT))
        return SetError(HPRT_E_INVALID, "hprt_debug_device_bsdf_specular: bad argument");
    HIP_TRY(hipSetDevice(s->device));
    SceneCall call(s, nullptr);
    const size_t nShapes = s->dev.nShapes, nMaterials = s->materials.bytes / sizeof(DevMaterial);
    if (s->shapes.bytes < nShapes * sizeof(DevShape)) return SetError(HPRT_E_INVALID, "hprt_debug_device_bsdf_specular: the scene has no shape table");
    std::vector<DevShape> shapes(nShapes);
    std::vector<DevMaterial> materials(nMaterials);
    if (nShapes) HIP_TRY(hipMemcpy(shapes.data(), s->shapes.p, nShapes * sizeof(DevShape), hipMemcpyDeviceToHost));
    if (nMaterials) HIP_TRY(hipMemcpy(materials.data(), s->materials.p, nMaterials * sizeof(DevMaterial), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) {
        if (shape[i] < 0 || (size_t)shape[i] >= nShapes) return SetError(HPRT_E_INVALID, "hprt_debug_device_bsdf_specular: shape index outside the scene");
        const int32_t mi = shapes[shape[i]].material;
        if (mi < 0 || (size_t)mi >= nMaterials) return SetError(HPRT_E_INVALID, "hprt_debug_device_bsdf_specular: the shape has no material");
        const DevMaterial &m = materials[mi];
        if (m.KdTex >= 0 || m.KsTex >= 0 || (m.type == 6 && m.opTex >= 0))
            return SetError(HPRT_E_INVALID, "hprt_debug_device_bsdf_specular: the shape's material has an image texture");
    }
    DevBuf dShape, dFrame, dWo, dU, dOut;
    HIP_TRY(dShape.alloc(n * sizeof(int32_t))); HIP_TRY(dFrame.alloc(n * 9 * sizeof(float))); HIP_TRY(dWo.alloc(n * 3 * sizeof(float)));
    HIP_TRY(dU.alloc(n * 2 * sizeof(float))); HIP_TRY(dOut.alloc(n * 8 * sizeof(float)));
    HIP_TRY(hipMemcpy(dShape.p, shape, n * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dFrame.p, frame9, n * 9 * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dWo.p, wo3, n * 3 * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dU.p, u2, n * 2 * sizeof(float), hipMemcpyHostToDevice));
    k_bsdf_specular_probe<<<dim3((unsigned)((n + 255) / 256)), dim3(256)>>>(s->dev, mask, n, dShape.as<int32_t>(), dFrame.as<float>(), dWo.as<float>(), dU.as<float>(),
                                                                            dOut.as<float>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out8, dOut.p, n * 8 * sizeof(float), hipMemcpyDeviceToHost));
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
