// hprt device side — kernel parameter blocks and launcher prototypes (kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <type_traits>
#include "dev_shading.h"

namespace hprt {

// Path data lives in HBM as STREAMS of 16-byte words: a lane reads or writes a whole word with
// one request, and a shading pass writes its results at its own thread index, so consecutive
// lanes touch consecutive words.  Index spaces are re-made every bounce: the paths that a bounce
// shades are numbered 0..n-1 in shading order (matte bin, plastic bin, generic bin) and
// everything that bounce produces — the next path segment, the shadow and MIS rays, the pending
// light terms — is stored under that number; queues list the numbers that need a given pass
// (in ascending runs, one per workgroup), so gathers stay almost sequential however thin the
// paths become.
struct RayStream { float4 *a, *b; };                 // a = {o.xyz, tMax}   b = {d.xyz, aux}
// A closest hit is ONE 16-byte word: everything shading needs of a hit in a scene without object instances.  `word` is the hit's
// primitive word (dev_scene.h: primitive index, shading bin in the high bits; negative: the ray escaped).  b carries what only some
// callers read — the ray-call entry points return t, scenes with object instances need the instance — and is null for everybody else
// (kernel-uniform): an accepted hit is then one store in the walk and one gather in k_shade.
struct HitStream { float4 *a; float2 *b; };           // a = {b0, b1, b2, word}   b = {t, instance or -1}; b may be null
// The layout lives in these helpers alone: every writer stores through hit_store / hit_store_miss, every reader loads a record
// (hit_load, hit_load_aux) and names its fields through the accessors.
__device__ __forceinline__ void hit_store(const HitStream &h, uint32_t slot, int32_t word, float b0, float b1, float b2, float t, int32_t inst) {
    h.a[slot] = make_float4(b0, b1, b2, __int_as_float(word));
    if (h.b) h.b[slot] = make_float2(t, __int_as_float(inst));
}
// (t of a miss: the ray's tMax, as Aggregate::Intersect leaves it)
__device__ __forceinline__ void hit_store_miss(const HitStream &h, uint32_t slot, float tMax) { hit_store(h, slot, -1, 0.f, 0.f, 0.f, tMax, -1); }
__device__ __forceinline__ float4 hit_load(const HitStream &h, uint32_t slot) { return h.a[slot]; }
__device__ __forceinline__ float2 hit_load_aux(const HitStream &h, uint32_t slot) { return h.b[slot]; }      // (h.b non-null)
__device__ __forceinline__ float2 hit_no_aux() { return make_float2(0.f, __int_as_float(-1)); }               // what a scene without instances would hold
// (the accessors also serve records copied to the host: TraceHost)
__host__ __device__ __forceinline__ int32_t hit_word(const float4 &rec) { return __builtin_bit_cast(int32_t, rec.w); }
__host__ __device__ __forceinline__ float hit_b0(const float4 &rec) { return rec.x; }
__host__ __device__ __forceinline__ float hit_b1(const float4 &rec) { return rec.y; }
__host__ __device__ __forceinline__ float hit_b2(const float4 &rec) { return rec.z; }
__host__ __device__ __forceinline__ float hit_t(const float2 &aux) { return aux.x; }
__host__ __device__ __forceinline__ int32_t hit_inst(const float2 &aux) { return __builtin_bit_cast(int32_t, aux.y); }
struct PathStream {
    RayStream ray;          // current path segment; ray.b.w = sampler dimension (bits 0-15) | bounces (bits 16-29) | RAY_FOLD_MARK (bit 30) | the segment left a specular lobe (bit 31)
    float4 *beta;           // {beta.rgb, path id}   path id = sampleInBatch * nPix + pixel
    float4 *L;              // {L.rgb, w}: w = 0 if the path ends at this vertex, else its etaScale (1 until it crosses a dielectric boundary)
};
// Fields of ray.b.w.  The bounce count keeps 14 bits (CheckDepth bounds maxdepth at 123).  RAY_FOLD_MARK: the vertex this segment leaves
// is a speculated one whose repair is left to the segment's reader (RenderParams::foldRepair) — only then does vs.occluded[that vertex]
// mean anything to the reader: a vertex without a shadow ray leaves the byte of an earlier bounce or batch there.
enum : uint32_t { RAY_DIM_MASK = 0xffffu, RAY_BOUNCE_SHIFT = 16u, RAY_BOUNCE_MASK = 0x3fffu, RAY_FOLD_MARK = 0x40000000u, RAY_SPECULAR = 0x80000000u };
// What a shading pass leaves for the rest of its bounce, indexed like its output PathStream
struct VertexStreams {
    RayStream shadow; uint8_t *occluded;             // shadow ray of the light sample, its any-hit result
    RayStream mis; HitStream misHit;                 // BSDF-sampled MIS ray, its closest hit (k_resolve: word, barycentrics)
    // A vertex with an MIS ray — every vertex with a pending term where RenderParams::speculate is off — is a FULL vertex: it leaves the
    // three pending streams and a resolve entry, and k_resolve adds its direct lighting once the rays are traced.
    float4 *pendLight;      // {light-sampling term rgb, info}   info: light number | bit30 shadow ray issued | bit31 MIS ray issued
    float4 *pendMis;        // {BSDF-sampling term rgb, light pick pdf}
    float4 *pendBeta;       // {beta before this vertex rgb, path id}
    // A SPECULATED vertex (a shadow ray and no MIS ray, RenderParams::speculate on) leaves one record in pendBeta instead and nothing in the
    // other two streams or the resolve queue: {radiance if the shadow ray is blocked rgb, path id | SPEC_RECORD | SPEC_END if the path ends
    // here}.  Its radiance if the ray is not blocked is already in out.L[j] (in Lfinal[path id] if the path ends here).  Where the ray has
    // turned out blocked the record's value stands for it: k_repair puts it there, or — RenderParams::foldRepair, for a vertex whose path
    // goes on — the next bounce's reader of out.L[j] (k_shade, k_bin) takes the record instead (RAY_FOLD_MARK).
    // pendBeta is one of two planes, alternated by bounce parity like the path streams: the readers of bounce b + 1 find bounce b's records
    // in pendPrev while k_shade(b + 1) writes its own at unrelated indices.  occluded needs no second plane: the any-hit walk of b + 1
    // writes it after those readers have run.
    const float4 *pendPrev;
};
// Flag bits of a speculated vertex's record word.  Path ids stay below 2^28: a batch holds at most 256 M paths (ChooseBatch), and RunBatch
// keeps a larger one (a caller's spp_chunk) on the full path.
enum : uint32_t { SPEC_RECORD = 0x80000000u, SPEC_END = 0x40000000u, SPEC_ID_MASK = 0x0fffffffu, SPEC_MAX_PATHS = 1u << 28 };
// end (RenderParams::foldRepair): the speculated vertices at which a path ends — no later reader, so k_repair runs over these alone
struct QueueSet {
    uint32_t *next, *shadow, *mis, *resolve, *end;
    uint32_t *nextCount, *shadowCount, *misCount, *resolveCount, *endCount;
};
// material bins (BIN_*, dev_scene.h): 0 matte, 1 plastic, 2 generic, 3 generic on an image-textured material (the variant compiled
// with the MIPMap lookups: scenes with textures only), 4 substrate.  count[k * BIN_STRIDE], k = 0..4: sizes; k = 5: size of bin 2
// before the specialised variants deferred vertices to it (counters 256 bytes apart: atomics on different bins do not share a line);
// k = 6, 7: the retry lists; aux[k] = output index of a deferred entry k of bin 2.  Output indices: bin 0 occupies [0, n0), then
// bins 1, 4, 2 (as binned) and 3.  A bin entry is {stream index, the hit's primitive word}: k_bin has the word in registers, and k_shade
// then requests the primitive record together with the path's streams instead of one memory round trip after them.
enum : uint32_t { BIN_STRIDE = 64u };
// retry[b - 2], b = 2, 3: {stream index, output index} pairs of vertices whose light-distribution voxel was not there yet
// (on-demand SpatialLightDistribution): shaded again by bin b's variant after the voxels have been filled; count[(6 + b - 2) * BIN_STRIDE]
struct BinSet { uint2 *q[5]; uint32_t *aux; uint32_t *count; uint2 *retry[2]; };
struct RenderParams {
    DevCamera cam;
    DevHalton hal;
    const uint32_t *pixelXY;        // x | y << 16 of every local pixel, tile by tile
    const uint64_t *pixelOffset;    // Halton index of sample 0: offsetForCurrentPixel (samplers/halton.cpp:101-118)
    uint32_t nPix;
    int32_t maxDepth;
    float rrThreshold;
    float invSqrtSpp;               // 1 / sqrt(samplesPerPixel): ray differential scale (image textures only)
    int32_t cullMis;                // do not trace rays whose result provably changes nothing (k_shade): a BSDF-sampled light ray that
                                    // cannot reach its emitter, the segment behind the last vertex of a path
    int32_t speculate;              // k_shade adds the light sample of a vertex with a shadow ray and no MIS ray at once (k_repair undoes the
                                    // blocked ones); 0: every such vertex goes through the pending streams and k_resolve
    int32_t foldRepair;             // (with speculate) a blocked speculated vertex whose path goes on is repaired by the next bounce's reader of its
                                    // radiance (RAY_FOLD_MARK); k_repair handles QueueSet::end only.  0: every shadow ray through k_repair, no mark
};
struct FilmGeom {
    int32_t cx0, cy0, cx1, cy1;     // croppedPixelBounds
    int32_t sx0, sy0, sx1, sy1;     // sample bounds
    float rx, ry;                   // filter radius
    float maxSampleLuminance;
};
struct IrregularSample { uint32_t pix, sample; int16_t x0, x1, y0, y1; };
// k_generate forms every camera sample's film position anyway: given this it also lists the irregular ones of its batch (count is
// cumulative over the batches of a render; entries beyond capacity are counted, not stored — the host then falls back to k_find_irregular)
struct IrregularSink { FilmGeom fg; uint32_t *count; uint32_t capacity; IrregularSample *out; };
// Samples that also land in pixels other than their own, grouped per destination.
struct FilmExtras {
    // same-tile: CSR over local pixels; entries sorted in the tile loop's order, pre first
    const uint32_t *ownBegin; const uint32_t *ownSrcPix; const uint32_t *ownSample; const uint8_t *ownIsPre;
    // other-tile: destinations -> groups (one per source tile) -> entries
    uint32_t nForeignDest;
    const uint32_t *foreignDestFilmIndex; const uint32_t *foreignDestBegin; const uint32_t *foreignGroupBegin;
    const uint32_t *foreignSrcPix; const uint32_t *foreignSample;
};

// One cross-tile film contribution (HprtFilmRecord of include/hprt.h): the fold of one source tile's samples that land in
// film pixel `dest` of another tile
struct FilmRecord { uint32_t dest, srcTile; float xyz[3]; float w; };

bool TraceProfileInUse();                    // the traversal kernels run their phase-profile variants (HPRT_TRACE_PROFILE, hprt_debug_trace_profile_mode)
bool WideWalkInUse(const DevScene &sc);      // plain renders of this scene take k_walk4 (the leaf-exact wide walk) rather than k_trace
void LaunchTrace(hipStream_t st, const DevScene &sc, bool anyHit, bool count, const uint32_t *queue, const uint32_t *countPtr,
                 uint32_t countImm, uint32_t gridItems, const RayStream &rays, const HitStream &hits, uint8_t *occ,
                 DevCounters *counters, uint32_t *workCounter, uint4 *rayStats = nullptr);
// Host side of the tree walks' launchers (kd_walk.hip, rbsp_walk.hip, rbspkd_walk.hip), each called from the file that defines its
// kernel: the work counter reset, the persistent grid (as many BLOCK-thread workgroups per CU on 256 CUs as the variant is
// compiled for, WAVES or QUAD_WAVES, never more than the rays need) and the pick of the kernel's <ANY_HIT, COUNT, QUAD>
// instantiation: launch(grid, block, std::integral_constant<bool, ANY_HIT>, ..COUNT, ..QUAD) starts it.
template <uint32_t BLOCK, uint32_t WAVES, uint32_t QUAD_WAVES, typename Launch>
void LaunchTreeWalk(hipStream_t st, const DevScene &sc, bool anyHit, bool count, uint32_t gridItems, uint32_t *workCounter, Launch launch) {
    if (gridItems == 0) return;
    (void)hipMemsetAsync(workCounter, 0, sizeof(uint32_t), st);
    const bool quad = sc.nSpheres != 0u;
    const dim3 grid(std::min((uint32_t)(((size_t)gridItems + BLOCK - 1) / BLOCK), 256u * (quad ? QUAD_WAVES : WAVES))), block(BLOCK);
    auto pickQuad = [&](auto a, auto c) { if (quad) launch(grid, block, a, c, std::true_type{}); else launch(grid, block, a, c, std::false_type{}); };
    auto pickCount = [&](auto a) { if (count) pickQuad(a, std::true_type{}); else pickQuad(a, std::false_type{}); };
    if (anyHit) pickCount(std::true_type{}); else pickCount(std::false_type{});
}
void LaunchPixelStats(hipStream_t st, const uint4 *rayStats, const float4 *ids, const uint32_t *queue, const uint32_t *countPtr,
                      uint32_t countImm, uint32_t gridItems, uint32_t nPix, bool anyHit, uint32_t *pix);
void LaunchPixelStatsToFilm(hipStream_t st, const uint32_t *pix, const uint32_t *pixelXY, uint32_t nPix, uint32_t spp, int cx0, int cy0, int width,
                            unsigned long long *out7);
void LaunchGenerate(hipStream_t st, const DevScene &sc, const RenderParams &rp, const PathStream &out, uint32_t s0, uint32_t nSlots,
                    const IrregularSink *irr = nullptr);
void LaunchBin(hipStream_t st, const DevScene &sc, const PathStream &in, const HitStream &hit, const uint32_t *queue,
               const uint32_t *countPtr, uint32_t countImm, uint32_t gridItems, int32_t maxDepth, int32_t bounces, const BinSet &bins,
               float4 *Lfinal, const VertexStreams &vs, bool foldRepair);
void LaunchShade(hipStream_t st, int mode, const DevScene &sc, const RenderParams &rp, const PathStream &in, const HitStream &hit,
                 uint32_t gridItems, uint32_t s0, const PathStream &out, const VertexStreams &vs, const QueueSet &q,
                 const BinSet &bins, float4 *Lfinal, bool firstBounce, bool retryPass = false);
void LaunchResolve(hipStream_t st, const DevScene &sc, const VertexStreams &vs, float4 *L, float4 *Lfinal, const uint32_t *queue,
                   const uint32_t *countPtr, uint32_t gridItems);
// queue: the bounce's shadow rays, or (RenderParams::foldRepair) its QueueSet::end.  counts (tests only, else null): {speculated, repaired} += this launch's
void LaunchRepair(hipStream_t st, const VertexStreams &vs, float4 *L, float4 *Lfinal, const uint32_t *queue, uint32_t n, uint32_t *counts);
void LaunchStoreRadiance(hipStream_t st, const float4 *Lfinal, float *LallR, float *LallG, float *LallB, uint32_t nPix, uint32_t s0,
                         uint32_t nSlots);
// the *_device entry points of include/hprt.h keep their plane layouts: [7][n] rays in, t / prim / [3][n] barycentrics out
void LaunchPackRays(hipStream_t st, const float *rays7, uint32_t n, const RayStream &out);
void LaunchUnpackHits(hipStream_t st, const HitStream &hits, uint32_t n, float *t, int32_t *prim, float *bary3);   // instance ids stay in hits.b
void LaunchFindIrregular(hipStream_t st, const DevScene &sc, const RenderParams &rp, const FilmGeom &fg, uint32_t spp, uint32_t *count,
                         uint32_t capacity, IrregularSample *out);
void LaunchFilmOwn(hipStream_t st, const RenderParams &rp, const FilmGeom &fg, const float *LallR, const float *LallG, const float *LallB,
                   uint32_t spp, const FilmExtras &ex, float *film);
void LaunchFilmForeign(hipStream_t st, const RenderParams &rp, const FilmGeom &fg, const float *LallR, const float *LallG,
                       const float *LallB, const FilmExtras &ex, float *film);
void LaunchFilmForeignExport(hipStream_t st, const RenderParams &rp, const FilmGeom &fg, const float *LallR, const float *LallG,
                             const float *LallB, const FilmExtras &ex, uint32_t nGroups, const uint32_t *groupDest, const uint32_t *groupTile,
                             FilmRecord *out);
// SpatialLightDistribution for every voxel: ri = RadicalInverse(0..4, i), i < 128, as [5][128] floats on the device
void LaunchVoxelDistributions(hipStream_t st, const DevScene &sc, const float *ri, uint32_t nVox, float *func, float *cdf, float *funcInt);
// on-demand mode: the `n` voxels listed in sc.voxRequest get rows rowBase .. rowBase + n - 1 (voxSlot is updated), their distributions are computed
void LaunchVoxelFill(hipStream_t st, const DevScene &sc, const float *ri, uint32_t n, uint32_t rowBase, float *func, float *cdf, float *funcInt);
void LaunchStreamCopy(hipStream_t st, const float4 *src, float4 *dst, size_t n);
void LaunchGatherProbe(hipStream_t st, const uint4 *records, uint32_t log2Records, int itersPerLane, uint32_t blocks, uint32_t *sink);
// diagnostics: the rays a queue lists, as [7][cap] planes (the layout of the *_device entry points)
void LaunchCaptureRays(hipStream_t st, const uint32_t *queue, uint32_t n, const RayStream &rays, float *out7, uint32_t cap);
void LaunchFilmApplyRecords(hipStream_t st, const FilmRecord *rec, const uint32_t *destBegin, uint32_t nDest, float *film);

}  // namespace hprt
