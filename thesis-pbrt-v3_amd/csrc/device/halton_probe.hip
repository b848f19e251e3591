// hprt — k_halton_probe: halton_dim (dev_shading.h) evaluated on gfx950 over host arrays of (index, dimension) pairs, so that a
// test can hold the device sampler against the oracle's HaltonSampler::SampleDimension directly — every dimension, indices on both
// sides of 2^32 — rather than through the few (index, dimension) pairs a render happens to draw.  Both forms of a dimension are
// reachable: the HBM tables (k_generate, k_find_irregular and every dimension from HPRT_HALTON_LDS_DIMS up) and the workgroup's
// LDS copy that k_shade stages with halton_lds_load.
//
// A translation unit of its own with a pinned CUID (build.py), linked into a library of its own (libhprt_probe.so, beside
// libhprt.so and linked against it): libhprt.so's code objects, and with them the stamp of the committed counter summaries, stay
// byte for byte what they were.  Diagnostics only; not part of include/hprt.h.
#include <hip/hip_runtime.h>
#include <string>
#include <vector>
#include "../../../include/hprt.h"
#include "../device_state.h"
#include "../halton_tables.h"
#include "dev_shading.h"

namespace hprt {
namespace {

__global__ __launch_bounds__(256) void k_halton_probe(DevScene sc, DevHalton hal, int useLds, size_t n, const uint64_t *__restrict__ index,
                                                       const int32_t *__restrict__ dim, float *__restrict__ out) {
    __shared__ HaltonLds hl;
    if (useLds) halton_lds_load(sc, &hl);      // (uniform per launch: every thread reaches the barrier inside)
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = halton_dim(sc, hal, index[i], dim[i], useLds ? &hl : nullptr);
}

}  // namespace
}  // namespace hprt

using namespace hprt;

// Diagnostics hook: out[i] = halton_dim(index[i], dim[i]) of a sampler over bounds_w x bounds_h sample bounds (the layout SetupFrame
// makes of them), read from the scene's own table buffers; use_lds != 0: through the LDS copy, as k_shade reads dimensions below
// HPRT_HALTON_LDS_DIMS.  Every dim must lie in [0, kPrimeTableSize): the tables end there.
extern "C" __attribute__((visibility("default"))) int hprt_debug_device_halton(HprtScene *s, int bounds_w, int bounds_h, int sample_pixel_center, int use_lds,
                                                                                 size_t n, const uint64_t *index, const int32_t *dim, float *out) try {
    if (!s || !index || !dim || !out || n == 0 || n > ((size_t)1 << 26) || bounds_w <= 0 || bounds_h <= 0)
        return SetError(HPRT_E_INVALID, "hprt_debug_device_halton: bad argument");
    for (size_t i = 0; i < n; ++i)
        if (dim[i] < 0 || dim[i] >= kPrimeTableSize) return SetError(HPRT_E_INVALID, "hprt_debug_device_halton: dimension outside the prime table");
    HIP_TRY(hipSetDevice(s->device));
    SceneCall call(s, nullptr);
    const HaltonLayout lay = MakeHaltonLayout(bounds_w, bounds_h);
    DevHalton hal;
    hal.baseScale1 = lay.baseScales[1]; hal.baseExp0 = lay.baseExponents[0]; hal.sampleStride = lay.sampleStride;
    hal.samplePixelCenter = sample_pixel_center;
    DevBuf dIndex, dDim, dOut;
    HIP_TRY(dIndex.alloc(n * sizeof(uint64_t))); HIP_TRY(dDim.alloc(n * sizeof(int32_t))); HIP_TRY(dOut.alloc(n * sizeof(float)));
    HIP_TRY(hipMemcpy(dIndex.p, index, n * sizeof(uint64_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dDim.p, dim, n * sizeof(int32_t), hipMemcpyHostToDevice));
    k_halton_probe<<<dim3((unsigned)((n + 255) / 256)), dim3(256)>>>(s->dev, hal, use_lds, n, dIndex.as<uint64_t>(), dDim.as<int32_t>(), dOut.as<float>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, dOut.p, n * sizeof(float), hipMemcpyDeviceToHost));
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
