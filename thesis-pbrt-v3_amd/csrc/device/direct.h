// hprt device side — the direct-lighting estimator (direct.hip): DirectLightingIntegrator::Li (integrators/directlighting.cpp:62-100)
// with UniformSampleAllLights / UniformSampleOneLight / EstimateDirect (core/integrator.cpp:55-217) and the recursion through
// SpecularReflect / SpecularTransmit (core/integrator.cpp:362-450), between the closest-hit traces of a batch's tree nodes and the
// any-hit and closest-hit traces of their light work.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels.h"

namespace hprt {

enum : uint32_t { DL_MAX_DEPTH = 8u,              // HPRT_DIRECT_MAX_DEPTH of include/hprt.h
                  DL_STACK_PLANES = 8u,           // 16-byte words per depth and camera sample (below)
                  DL_RECORD_PLANES = 4u,          // 16-byte words per hit record
                  DL_MAX_ITEMS = 1u << 16 };      // light samples per node: the sum of the lights' sample counts

// What the kernels of one render share (kernel-uniform)
struct DlParams {
    int32_t strategy;                  // 0 "all" (UniformSampleAllLights), 1 "one" (UniformSampleOneLight)
    int32_t maxDepth;
    uint32_t nLights;
    uint32_t itemsPerHit;              // lanes of k_dl_rays per hit: "all": the sum of nLightSamples (>= nLights), "one": 1
    int32_t arrayEndDim;               // 5 + 4 * maxDepth * nLights ("all"), 5 ("one"): the first plain dimension behind the sample arrays
    const int32_t *nLightSamples;      // [nLights]
    const uint32_t *lightFirstItem;    // [nLights]: light j's samples are items lightFirstItem[j] .. + nLightSamples[j] - 1
    const uint2 *itemLight;            // [itemsPerHit] ("all"): {light, k} of an item
};

// Which camera sample a slot of the batch is: sample (s0 + slot / nPix) of pixel slot % nPix, or — hprt_sample_direct — sampleNum[slot]
// of the pixel whose Halton offset is pixelBase[slot].  pixelBase: offsetForCurrentPixel (samplers/halton.cpp:101-118).
struct DlSlots { const uint64_t *pixelBase; const uint32_t *sampleNum; uint32_t nPix, s0; };

// Per camera sample (slot) of a batch:
//   state[slot]   the sampler's two cursors and the walk's position: dimension (bits 0-15) | depth of the current node (16-19) |
//                 nodes that have drawn their sample arrays so far (20-27) — array2DOffset / (2 * nLights) of core/sampler.cpp:93-98
//   stack         per depth d, DL_STACK_PLANES planes of 16-byte words `stride` apart (plane (d * 8 + k), word slot):
//     0 {L of the node so far rgb, phase}        phase 0: SpecularReflect next, 1: SpecularTransmit next, 2: the node is complete
//     1 {f rgb, AbsDot(wi, ns)}  2 {p, pdf}      of the specular child being walked (f * Li * AbsDot / pdf, core/integrator.cpp:394, 446)
//     3 {pError, material}  4 {wo, -}  5 {n, -}  6 {shading.n, -}  7 {shading.dpdu, -}      the node's SurfaceInteraction
struct DlState { uint32_t *state; float4 *stack; uint32_t stride; };

// One record per node that hit a surface in this step, numbered in the order k_dl_shade appended them (planes `stride` apart):
//   0 {slot, depth | mode << 8 | texture flags << 16, dimBase, array node}   mode 0: sample arrays, 1: the single-sample fallback
//     (core/integrator.cpp:67-72), 2: UniformSampleOneLight; dimBase: the dimension of the node's first plain light sample value;
//     texture flags: bit 0 Kd, 1 Ks, 2 opacity evaluated (planes 1-3)
//   1-3 the evaluated image textures of Kd, Ks and opacity at the hit (camera-ray hits only: a spawned ray has no differentials)
struct DlRecords { uint4 *q; float4 *tex; uint32_t stride; };

// The light work of a range of hits [h0, h0 + nh): item `it` of hit h0 + hl is entry it * nh + hl (consecutive lanes, consecutive
// hits).  a = {light-sampling term rgb, index of its shadow ray or -1}, b = {BSDF-sampling term rgb, index of its ray or -1 (bit 30:
// the ray is traced, as the reference traces it, but its light is black)}, light = the item's light ("one": the light Get1D picked)
struct DlItems { float4 *a, *b; uint32_t *light; };
struct DlRays { RayStream shadow; uint8_t *occ; RayStream bsdf; HitStream bsdfHit; uint32_t *shadowCount, *bsdfCount; };

// The per-sample radiance store of a render (k_store_radiance's): Lall[channel][sample][pixel]; base = index of the batch's slot 0
struct DlRadiance { float *R, *G, *B; size_t base; };

// k_dl_shade: one lane per live node i (slot = live ? live[i] : i, its ray rays[i], its closest hit hit[i]).  first: step 0 of a
// batch — the nodes are the camera rays and their state is formed here, not read.
void LaunchDlShade(hipStream_t st, const DevScene &sc, const RenderParams &rp, const DlParams &dp, const DlSlots &sl, const RayStream &rays,
                   const HitStream &hit, const uint32_t *live, uint32_t nLive, bool first, const DlState &state, const DlRecords &recs, uint32_t *hitCount);
// k_dl_rays: one lane per (hit, item) of the hits [h0, h0 + nh): EstimateDirect's two halves up to their rays
void LaunchDlRays(hipStream_t st, const DevScene &sc, const RenderParams &rp, const DlParams &dp, const DlSlots &sl, const DlState &state,
                  const DlRecords &recs, uint32_t h0, uint32_t nh, const DlItems &items, const DlRays &rays);
// k_dl_resolve: one lane per hit of the range: the estimates summed in the reference's order into the node's L
void LaunchDlResolve(hipStream_t st, const DevScene &sc, const DlParams &dp, const DlState &state, const DlRecords &recs, uint32_t h0, uint32_t nh,
                     const DlItems &items, const DlRays &rays);
// k_dl_advance: one lane per live node: SpecularReflect / SpecularTransmit of the node or of the ancestors its completion returns to;
// a sample either leaves its next node's ray in `next` (and its slot in nextLive) or its radiance in `out`
void LaunchDlAdvance(hipStream_t st, const DevScene &sc, const RenderParams &rp, const DlParams &dp, const DlSlots &sl, const uint32_t *live,
                     uint32_t nLive, const DlState &state, const RayStream &next, uint32_t *nextLive, uint32_t *nextCount, const DlRadiance &out);

}  // namespace hprt
