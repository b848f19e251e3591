// hprt device side — the ambient-occlusion estimator (ao.hip): AOIntegrator::Li (integrators/ao.cpp:57-103) between the closest-hit
// trace of a batch of camera samples and the any-hit trace of their hemisphere rays.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels.h"

namespace hprt {

// One record per camera sample that hit, numbered in the order k_ao_frame appended them, as five planes of 16-byte words `stride`
// apart (a plane is written and read by consecutive lanes):
//   plane 0  {p.xyz, camera slot}                    plane 1  {pError.xyz, 0}
//   plane 2  {isect.n.xyz, 1 if Faceforward(isect.n, -ray.d) flipped it, else 0}
//   plane 3  {s.xyz, low word}  plane 4  {t.xyz, high word}  of the Halton index of the hit's first array sample,
//            GetIndexForSample(pixel sample * nSamples) (core/sampler.cpp:154-164)
struct AoRecords { float4 *rec; uint32_t stride; };
enum : uint32_t { AO_RECORD_PLANES = 5u, AO_MAX_SAMPLES = 1024u };

// The per-sample radiance store of a render (k_store_radiance's): Lall[channel][sample][pixel]; base = index of the batch's slot 0
struct AoRadiance { float *R, *G, *B; size_t base; };

// k_ao_frame: one lane per camera sample of the batch.  aoBase (or null): the Halton index of array sample 0 of slot i's camera sample,
// for callers whose slots are not (sample s0 + slot / nPix of pixel slot % nPix) — hprt_sample_ao
void LaunchAoFrame(hipStream_t st, const DevScene &sc, const RenderParams &rp, const RayStream &rays, const HitStream &hit, uint32_t nSlots, uint32_t s0,
                   uint32_t nSamples, const uint64_t *aoBase, const AoRecords &recs, uint32_t *hitCount, const AoRadiance &out);
// k_ao_rays: one lane per hemisphere ray r = hit * nSamples + i of the hits [h0, h0 + nHits); ray r - h0 * nSamples is written at index
// r - h0 * nSamples of `out` and `term`
void LaunchAoRays(hipStream_t st, const DevScene &sc, const DevHalton &hal, const AoRecords &recs, uint32_t h0, uint32_t nHits, uint32_t nSamples,
                  bool cosSample, const RayStream &out, float *term);
// k_ao_resolve: one lane per hit of [h0, h0 + nHits): the terms of its unoccluded rays added in the order i = 0 .. nSamples - 1, the
// radiance guards (core/integrator.cpp:300-321), and the store where k_store_radiance would put the sample
void LaunchAoResolve(hipStream_t st, const AoRecords &recs, uint32_t h0, uint32_t nHits, uint32_t nSamples, const uint8_t *occ, const float *term,
                     const AoRadiance &out);

}  // namespace hprt
