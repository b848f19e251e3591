// hprt — k_bsdf_probe: bsdf_init, bsdf_f, bsdf_pdf and bsdf_sample (dev_shading.h) evaluated on gfx950 over host arrays of
// (shape, frame, wo, wi, u) queries, so that a test can hold the device's hand-fused BSDF against the oracle's lobe-array BSDF
// (oracle/orc_shading.h) directly — every material, every branch, the inputs a render forms seldom or never — rather than through
// the few (material, wo, wi, u) a film's paths happen to form.  No texture overrides: the material's constants.
//
// A translation unit of its own with a pinned CUID (build.py), linked into libhprt_probe.so beside halton_probe.hip: libhprt.so
// gains no code object.  Diagnostics only; not part of include/hprt.h.
#include <hip/hip_runtime.h>
#include <string>
#include <vector>
#include "../../../include/hprt.h"
#include "../device_state.h"
#include "dev_shading.h"

namespace hprt {
namespace {

// One query per thread.  frame9: n, ns (shading.n), sdpdu (shading.dpdu).  out8, unused words 0:
//   mode 0: material type, bsdf_num, eta          mode 1: bsdf_f (3)          mode 2: bsdf_pdf
//   mode 3 / 4: bsdf_sample with all = false / true: f (3), wiW (3), pdf, sampledType — pdf, wiW and sampledType preset to -7,
//   (9, 9, 9) and -1, so that the early returns that leave them untouched show
__global__ __launch_bounds__(256) void k_bsdf_probe(DevScene sc, int mode, size_t n, const int32_t *__restrict__ shape, const float *__restrict__ frame9,
                                                     const float *__restrict__ wo3, const float *__restrict__ wi3, const float *__restrict__ u2,
                                                     float *__restrict__ out8) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *fr = frame9 + 9 * i;
    DevSI si;
    si.p = vec3(0.f, 0.f, 0.f); si.pErr = vec3(0.f, 0.f, 0.f); si.wo = vec3(0.f, 0.f, 0.f);      // (unused by the BSDF)
    si.n = vec3(fr[0], fr[1], fr[2]); si.ns = vec3(fr[3], fr[4], fr[5]); si.sdpdu = vec3(fr[6], fr[7], fr[8]);
    si.shape = shape[i]; si.material = -1;
    DevBsdf b;
    bsdf_init(sc, si, &b);
    const vec3 wo(wo3[3 * i], wo3[3 * i + 1], wo3[3 * i + 2]), wi(wi3[3 * i], wi3[3 * i + 1], wi3[3 * i + 2]);
    float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (mode == 0) {
        o[0] = (float)sc.materials[si_material(sc, si)].type; o[1] = (float)bsdf_num(b); o[2] = b.eta;
    } else if (mode == 1) {
        const rgb f = bsdf_f(b, wo, wi);
        o[0] = f.r; o[1] = f.g; o[2] = f.b;
    } else if (mode == 2) {
        o[0] = bsdf_pdf(b, wo, wi);
    } else {
        float pdf = -7.0f; vec3 w(9.f, 9.f, 9.f); int sampledType = -1;
        const rgb f = mode == 3 ? bsdf_sample(b, wo, &w, u2[2 * i], u2[2 * i + 1], &pdf, &sampledType, false)
                                : bsdf_sample(b, wo, &w, u2[2 * i], u2[2 * i + 1], &pdf, &sampledType, true);
        o[0] = f.r; o[1] = f.g; o[2] = f.b; o[3] = w.x; o[4] = w.y; o[5] = w.z; o[6] = pdf; o[7] = (float)sampledType;
    }
    float4 *dst = (float4 *)(out8 + 8 * i);      // (hipMalloc'ed base, 32 bytes per query)
    dst[0] = make_float4(o[0], o[1], o[2], o[3]);
    dst[1] = make_float4(o[4], o[5], o[6], o[7]);
}

}  // namespace
}  // namespace hprt

using namespace hprt;

// Diagnostics hook: out8[8 * i ..] = the device BSDF of shapes[shape[i]]'s material at the frame frame9[9 * i ..] (n, shading.n,
// shading.dpdu), evaluated in `mode` (see k_bsdf_probe) for wo3 / wi3 / u2 [i].  Refused without a launch: a null pointer, n == 0 or
// n > 2^22, a mode outside 0..4, a shape index outside the scene's shapes, a shape whose material has an image texture on Kd, Ks
// or opacity (the probe passes bsdf_init no overrides).
extern "C" __attribute__((visibility("default"))) int hprt_debug_device_bsdf(HprtScene *s, int mode, size_t n, const int32_t *shape, const float *frame9,
                                                                               const float *wo3, const float *wi3, const float *u2, float *out8) try {
    if (!s || !shape || !frame9 || !wo3 || !wi3 || !u2 || !out8 || n == 0 || n > ((size_t)1 << 22) || mode < 0 || mode > 4)
        return SetError(HPRT_E_INVALID, "hprt_debug_device_bsdf: bad argument");
    HIP_TRY(hipSetDevice(s->device));
    SceneCall call(s, nullptr);
    // the scene keeps its shape and material tables on the device only: read them back for the checks
    const size_t nShapes = s->dev.nShapes, nMaterials = s->materials.bytes / sizeof(DevMaterial);
    if (s->shapes.bytes < nShapes * sizeof(DevShape)) return SetError(HPRT_E_INVALID, "hprt_debug_device_bsdf: the scene has no shape table");
    std::vector<DevShape> shapes(nShapes);
    std::vector<DevMaterial> materials(nMaterials);
    if (nShapes) HIP_TRY(hipMemcpy(shapes.data(), s->shapes.p, nShapes * sizeof(DevShape), hipMemcpyDeviceToHost));
    if (nMaterials) HIP_TRY(hipMemcpy(materials.data(), s->materials.p, nMaterials * sizeof(DevMaterial), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) {
        if (shape[i] < 0 || (size_t)shape[i] >= nShapes) return SetError(HPRT_E_INVALID, "hprt_debug_device_bsdf: shape index outside the scene");
        const int32_t mi = shapes[shape[i]].material;
        if (mi < 0 || (size_t)mi >= nMaterials) return SetError(HPRT_E_INVALID, "hprt_debug_device_bsdf: the shape has no material");
        const DevMaterial &m = materials[mi];
        if (m.KdTex >= 0 || m.KsTex >= 0 || (m.type == 6 && m.opTex >= 0))
            return SetError(HPRT_E_INVALID, "hprt_debug_device_bsdf: the shape's material has an image texture");
    }
    DevBuf dShape, dFrame, dWo, dWi, dU, dOut;
    HIP_TRY(dShape.alloc(n * sizeof(int32_t))); HIP_TRY(dFrame.alloc(n * 9 * sizeof(float))); HIP_TRY(dWo.alloc(n * 3 * sizeof(float)));
    HIP_TRY(dWi.alloc(n * 3 * sizeof(float))); HIP_TRY(dU.alloc(n * 2 * sizeof(float))); HIP_TRY(dOut.alloc(n * 8 * sizeof(float)));
    HIP_TRY(hipMemcpy(dShape.p, shape, n * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dFrame.p, frame9, n * 9 * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dWo.p, wo3, n * 3 * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dWi.p, wi3, n * 3 * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dU.p, u2, n * 2 * sizeof(float), hipMemcpyHostToDevice));
    k_bsdf_probe<<<dim3((unsigned)((n + 255) / 256)), dim3(256)>>>(s->dev, mode, n, dShape.as<int32_t>(), dFrame.as<float>(), dWo.as<float>(), dWi.as<float>(),
                                                                   dU.as<float>(), dOut.as<float>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out8, dOut.p, n * 8 * sizeof(float), hipMemcpyDeviceToHost));
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
