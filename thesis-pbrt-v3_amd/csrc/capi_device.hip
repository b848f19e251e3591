// hprt — device half of the C ABI (include/hprt.h): HBM scene upload, batched
// Intersect/IntersectP, the wavefront Render loop and the film.  Host-side
// orchestration only; the arithmetic lives in device/*.h and device/kernels.hip.
// There is no CPU fallback: every entry point fails with HPRT_E_NO_DEVICE when no
// HIP device is usable.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cassert>
#include <chrono>
#include <cmath>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>
#include "../../include/hprt.h"
#include "device/kernels.h"
#include "device/ao.h"
#include "device/direct.h"
#include "halton_tables.h"
#include "host_transform.h"
#include "hprt_internal.h"
#include "device_state.h"
#include "scene_layout.h"
#include "wide_bvh.h"

using namespace hprt;


namespace {

int CheckDevice(int device, int *chosen) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return SetError(HPRT_E_NO_DEVICE, "no HIP device available (hprt has no CPU fallback)");
    if (device < 0) { if (hipGetDevice(&device) != hipSuccess) device = 0; }
    if (device >= n) return SetError(HPRT_E_INVALID, "device ordinal out of range");
    if (hipSetDevice(device) != hipSuccess) return SetError(HPRT_E_DEVICE, "hipSetDevice failed");
    *chosen = device;
    return HPRT_OK;
}

struct PlaneAllocator {
    char *base; size_t off = 0, cap;
    template <typename T> T *take(size_t n) { off = (off + 255) & ~(size_t)255; T *p = (T *)(base + off); off += n * sizeof(T); return p; }
};
// Device view of one batch's path data (device/kernels.h): two path streams used alternately
// (a bounce reads one and writes the other), the hits of the stream being read, the per-vertex
// streams and the finished paths' radiance by path id.
struct Workspace {
    PathStream path[2];
    HitStream hit;
    VertexStreams vs;
    float4 *pend[2];        // the two planes of vs.pendBeta / vs.pendPrev: bounce b writes pend[b & 1] (RunBatch)
    float4 *Lfinal;
};
// 16-byte words per stream index: 2 x (ray a,b + beta + L) + hit a + shadow a,b + mis a,b + misHit a
// + pendLight/Mis + 2 x pendBeta + Lfinal; plus occluded (1 B) and alignment slack.  A render reads the second word of a hit record
// ({t, instance}, HitStream::b) for the instance alone, so only scenes with object instances get those planes (8 B each, path hit and MIS hit).
const size_t kPlaneBytesPerSlot = 16 * (2 * 4 + 1 + 2 + 2 + 1 + 4 + 1) + 1, kInstancePlaneBytesPerSlot = 8 + 8;
size_t PlaneBytesPerSlot(bool instances) { return kPlaneBytesPerSlot + (instances ? kInstancePlaneBytesPerSlot : 0); }
size_t PlaneBytes(size_t n, bool instances) { return n * PlaneBytesPerSlot(instances) + 32 * 256; }

void CarvePlanes(char *base, size_t n, bool instances, Workspace *w) {
    PlaneAllocator a{base, 0, 0};
    auto rays = [&](RayStream &r) { r.a = a.take<float4>(n); r.b = a.take<float4>(n); };
    for (int k = 0; k < 2; ++k) { rays(w->path[k].ray); w->path[k].beta = a.take<float4>(n); w->path[k].L = a.take<float4>(n); }
    w->hit.a = a.take<float4>(n); w->hit.b = instances ? a.take<float2>(n) : nullptr;
    rays(w->vs.shadow); w->vs.occluded = a.take<uint8_t>(n);
    rays(w->vs.mis); w->vs.misHit.a = a.take<float4>(n); w->vs.misHit.b = instances ? a.take<float2>(n) : nullptr;
    w->vs.pendLight = a.take<float4>(n); w->vs.pendMis = a.take<float4>(n);
    for (int k = 0; k < 2; ++k) w->pend[k] = a.take<float4>(n);
    w->vs.pendBeta = w->pend[0]; w->vs.pendPrev = w->pend[1];
    w->Lfinal = a.take<float4>(n);
}

struct EventTimer {
    std::vector<hipEvent_t> pool; size_t used = 0;
    ~EventTimer() { for (hipEvent_t e : pool) (void)hipEventDestroy(e); }
    hipEvent_t get() {
        if (used == pool.size()) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return nullptr; pool.push_back(e); }
        return pool[used++];
    }
    void reset() { used = 0; }
};

// Camera matrices: ProjectiveCamera ctor, core/camera.h:84-115
void MakeCamera(const HprtRenderOptions &o, DevCamera *cam) {
    Xform camToScreen = xf_perspective(o.fov, 1e-2f, 1000.f);
    const float *sw = o.screen_window;
    Xform screenToRaster = xf_scale((float)o.xres, (float)o.yres, 1) * xf_scale(1 / (sw[1] - sw[0]), 1 / (sw[2] - sw[3]), 1) *
                           xf_translate(vec3(-sw[0], -sw[3], 0));
    Xform rasterToScreen = screenToRaster.inverse();
    Xform rasterToCamera = camToScreen.inverse() * rasterToScreen;
    cam->rasterToCamera = rasterToCamera.m;
    memcpy(cam->cameraToWorld.m, o.camera_to_world, 64);
    cam->lensRadius = o.lens_radius; cam->focalDistance = o.focal_distance;
    // cameras/perspective.cpp:55-58
    cam->dxCamera = xf_point(cam->rasterToCamera, vec3(1, 0, 0)) - xf_point(cam->rasterToCamera, vec3(0, 0, 0));
    cam->dyCamera = xf_point(cam->rasterToCamera, vec3(0, 1, 0)) - xf_point(cam->rasterToCamera, vec3(0, 0, 0));
}

// A path vertex consumes up to 8 sampler dimensions after the camera sample's 5; the reference's
// Halton sampler aborts at dimension PrimeTableSize = 1000 (core/lowdiscrepancy.h:52, lowdiscrepancy.cpp:4558), so depths
// whose paths could get there are refused instead of sampled from a dimension the reference does not have.
int CheckDepth(int maxDepth) {
    if (5 + 8 * ((int64_t)maxDepth + 1) > 1000)
        return SetError(HPRT_E_UNSUPPORTED, "maxdepth above 123: a path could pass the 1,000 sampler dimensions of the reference's Halton tables");
    return HPRT_OK;
}

struct FrameSetup {
    FilmGeom fg; int ntx, nty; HaltonLayout hal; RenderParams rp;
    std::vector<uint32_t> pixelXY; std::vector<uint64_t> pixelOffset;
    std::vector<int32_t> localIndex;   // cropped-film index -> local pixel index or -1
    int W, H;
    // HaltonSampler::GetIndexForSample's per-pixel offset (samplers/halton.cpp:101-118) depends on the pixel
    // coordinates modulo kMaxResolution only: offset = (offX[x mod 128] + offY[y mod 128]) mod sampleStride
    uint64_t offX[128], offY[128];
};
int SetupFrame(const HprtRenderOptions &o, FrameSetup *f) {
    if (o.xres <= 0 || o.yres <= 0 || o.xres > 32768 || o.yres > 32768) return SetError(HPRT_E_INVALID, "film resolution out of range");
    if (o.filter_radius[0] != 0.5f || o.filter_radius[1] != 0.5f)
        return SetError(HPRT_E_UNSUPPORTED, "only the box filter with radius 0.5 is in the hot-path scope (SURVEY.md §2)");
    FilmGeom &fg = f->fg;
    fg.cx0 = (int)std::ceil(o.xres * o.crop[0]); fg.cx1 = (int)std::ceil(o.xres * o.crop[1]);   // core/film.cpp:56-60
    fg.cy0 = (int)std::ceil(o.yres * o.crop[2]); fg.cy1 = (int)std::ceil(o.yres * o.crop[3]);
    fg.rx = o.filter_radius[0]; fg.ry = o.filter_radius[1];
    fg.sx0 = (int)std::floor((float)fg.cx0 + 0.5f - fg.rx); fg.sy0 = (int)std::floor((float)fg.cy0 + 0.5f - fg.ry);   // core/film.cpp:81-87
    fg.sx1 = (int)std::ceil((float)fg.cx1 - 0.5f + fg.rx); fg.sy1 = (int)std::ceil((float)fg.cy1 - 0.5f + fg.ry);
    fg.maxSampleLuminance = o.max_sample_luminance;
    f->W = fg.cx1 - fg.cx0; f->H = fg.cy1 - fg.cy0;
    if (f->W <= 0 || f->H <= 0) return SetError(HPRT_E_INVALID, "empty crop window");
    f->ntx = (fg.sx1 - fg.sx0 + 15) / 16; f->nty = (fg.sy1 - fg.sy0 + 15) / 16;                   // core/integrator.cpp:237-239
    f->hal = MakeHaltonLayout(fg.sx1 - fg.sx0, fg.sy1 - fg.sy0);
    // the two addends of the offset (each already reduced), from the layout's own function on (m, 0) and (0, m)
    const uint64_t base = (uint64_t)HaltonPixelOffset(f->hal, 0, 0), stride = (uint64_t)std::max(1, f->hal.sampleStride);
    for (int m = 0; m < 128; ++m) {
        f->offX[m] = (uint64_t)HaltonPixelOffset(f->hal, m, 0);
        f->offY[m] = ((uint64_t)HaltonPixelOffset(f->hal, 0, m) + stride - base) % stride;
    }
    return HPRT_OK;
}
// a render's offset of pixel (x, y), from the two tables (hprt_debug_halton_index holds it against HaltonPixelOffset)
uint64_t TilePixelOffset(const FrameSetup &f, int x, int y) {
    const uint64_t stride = (uint64_t)std::max(1, f.hal.sampleStride);
    return f.hal.sampleStride > 1 ? (f.offX[((x % 128) + 128) % 128] + f.offY[((y % 128) + 128) % 128]) % stride : 0ull;
}
void AddTilePixels(FrameSetup *f, int tile) {
    const FilmGeom &fg = f->fg;
    int tx = tile % f->ntx, ty = tile / f->ntx;
    int x0 = fg.sx0 + tx * 16, x1 = std::min(x0 + 16, fg.sx1), y0 = fg.sy0 + ty * 16, y1 = std::min(y0 + 16, fg.sy1);
    for (int y = y0; y < y1; ++y)
        for (int x = x0; x < x1; ++x) {
            f->localIndex[(size_t)(y - fg.cy0) * f->W + (x - fg.cx0)] = (int32_t)f->pixelXY.size();
            f->pixelXY.push_back((uint32_t)x | ((uint32_t)y << 16));
            f->pixelOffset.push_back(TilePixelOffset(*f, x, y));
        }
}

}  // namespace

extern "C" {

int hprt_scene_create(const HprtSceneDesc *d, int device, HprtScene **out) try {
    if (!d || !out) return SetError(HPRT_E_INVALID, "hprt_scene_create: null argument");
    SceneLayout L;
    if (int rc = BuildSceneLayout(*d, &L)) return rc;
    int dev;
    if (int rc = CheckDevice(device, &dev)) return rc;
    std::unique_ptr<HprtScene> sc(new HprtScene());
    sc->device = dev; sc->nPrims = L.nPrims;
    sc->topOrder = std::move(L.topOrder); sc->objectOrder = std::move(L.objectOrder); sc->objectPrimBase = std::move(L.objectPrimBase);
    sc->instanceObject = std::move(L.instanceObject); sc->instanced = L.instanced; sc->hasSubstrateBin = L.hasSubstrateBin;
    for (const DevMaterial &m : L.materials) {      // (hprt_render_direct's refusals)
        if (m.KdTex >= 0 || m.KsTex >= 0 || (m.type == 6 && m.opTex >= 0)) sc->hasImageTexture = true;
        const bool uberLobe = m.type == 6 && (m.Kr[0] > 0 || m.Kr[1] > 0 || m.Kr[2] > 0 || m.Kt[0] > 0 || m.Kt[1] > 0 || m.Kt[2] > 0 || m.opTex >= 0 ||
                                              m.opacity[0] != 1.f || m.opacity[1] != 1.f || m.opacity[2] != 1.f);
        if (m.type == 2 || (m.type == 5 && !m.roughGlass) || uberLobe) sc->hasSpecularLobe = true;
    }
    // Halton tables + 64-bit division magics
    const std::vector<uint16_t> &perms = HaltonPermutations();
    std::vector<int32_t> primes(PrimeTable().begin(), PrimeTable().end()), primeSums(PrimeSumTable().begin(), PrimeSumTable().end());
    std::vector<uint64_t> magic(primes.size());
    for (size_t i = 0; i < primes.size(); ++i) magic[i] = 0xffffffffffffffffull / (uint64_t)primes[i] + 1ull;
    // ---- upload ----
    HIP_TRY(upload(sc->nodes, L.pairs)); HIP_TRY(upload(sc->tris, L.tris)); HIP_TRY(upload(sc->primVtx, L.primVtx));
    HIP_TRY(upload(sc->primN, L.primN)); HIP_TRY(upload(sc->vUV, L.vUV)); HIP_TRY(upload(sc->vS, L.vS));
    HIP_TRY(upload(sc->shapes, L.shapes)); HIP_TRY(upload(sc->materials, L.materials)); HIP_TRY(upload(sc->lights, L.lights));
    HIP_TRY(upload(sc->spheres, L.spheres)); HIP_TRY(upload(sc->instances, L.instances)); HIP_TRY(upload(sc->topEntry, L.topEntry));
    HIP_TRY(upload(sc->topEntryWide, L.topEntryWide)); HIP_TRY(upload(sc->lightFunc, L.lightFunc)); HIP_TRY(upload(sc->lightCdf, L.lightCdf));
    HIP_TRY(upload(sc->perms, perms)); HIP_TRY(upload(sc->primes, primes)); HIP_TRY(upload(sc->primeSums, primeSums));
    HIP_TRY(upload(sc->primeMagic, magic));
    HIP_TRY(upload(sc->textures, L.textures)); HIP_TRY(upload(sc->mipLevels, L.mipLevels)); HIP_TRY(upload(sc->texels, L.texels)); HIP_TRY(upload(sc->weightLut, L.weightLut));
    HIP_TRY(upload(sc->wide, L.wide)); HIP_TRY(upload(sc->leafBox, L.leafBox));
    HIP_TRY(upload(sc->envLights, L.envLights)); HIP_TRY(upload(sc->envData, L.envData));
    if (L.grid.lists.eligible) {
        const ShadowGrid &sg = L.grid.lists;
        const ShadowGridImage &im = L.gridImage;      // (the lists with their triangles in list order: shadow_grid.h)
        // blocks, then records, in one allocation (scene_layout.cpp keeps the image below 2^32 bytes)
        const size_t blockBytes = im.blocks.size() * sizeof(uint32_t), recordBytes = im.records.size() * sizeof(uint32_t);
        if (blockBytes + recordBytes > 0xffff0000ull)
            return SetError(HPRT_E_INVALID, L.gridKind == GridKind::Point ? "hprt_scene_create: the shadow grid's image is too large" : "hprt_scene_create: the distant grid's image is too large");
        HIP_TRY(sc->gridImage.alloc(blockBytes + recordBytes));
        HIP_TRY(hipMemcpy(sc->gridImage.p, im.blocks.data(), blockBytes, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy((char *)sc->gridImage.p + blockBytes, im.records.data(), recordBytes, hipMemcpyHostToDevice));
        sc->gridKind = L.gridKind;
        sc->grid = DevDistantGrid{sc->gridImage.as<uint32_t>(), (uint32_t)(blockBytes + recordBytes), (uint32_t)blockBytes, sg.nNear, sg.R, L.grid.frame};
        HprtScene::GridInfo &in = sc->gridInfo;
        in.nEntries = sg.entries.size(); in.longest = sg.longest; in.buildSeconds = sg.buildSeconds; in.packSeconds = im.packSeconds; in.eps = sg.eps; in.bytes = im.bytes();
        for (int a = 0; a < 3; ++a) in.light[a] = sg.light[a];
    }
    HIP_TRY(sc->counters.alloc(sizeof(DevCounters)));
    HIP_TRY(hipMemset(sc->counters.p, 0, sizeof(DevCounters)));
    HIP_TRY(sc->deepStack.alloc((size_t)HPRT_SPILL_STACK * HPRT_DEEP_THREADS * sizeof(uint2)));
    HIP_TRY(sc->workCounter.alloc(256));
    DevScene &dv = sc->dev;
    dv.pairs = sc->nodes.as<DevPair>(); dv.nPairs = (uint32_t)L.pairs.size();
    dv.wide = L.wide.empty() ? nullptr : sc->wide.as<DevWide>(); dv.nWide = (uint32_t)L.wide.size(); dv.leafBox = sc->leafBox.as<float4>();
    dv.tris = sc->tris.as<float4>(); dv.nPrims = L.nPrims;
    dv.primVtx = sc->primVtx.as<uint32_t>();
    dv.primN = sc->primN.as<float4>(); dv.vUV = sc->vUV.as<float>(); dv.vS = sc->vS.as<float>();
    dv.shapes = sc->shapes.as<DevShape>(); dv.nShapes = d->n_shapes;
    dv.materials = sc->materials.as<DevMaterial>();
    dv.lights = sc->lights.as<DevLight>(); dv.nLights = d->n_lights;
    dv.spheres = sc->spheres.as<DevSphere>(); dv.nSpheres = (uint32_t)L.spheres.size();
    dv.envLights = sc->envLights.as<DevEnvLight>(); dv.envData = sc->envData.as<float>(); dv.nEnvLights = (uint32_t)L.envLights.size();
    dv.textures = d->n_textures ? sc->textures.as<DevTexture>() : nullptr; dv.mipLevels = sc->mipLevels.as<DevMipLevel>();
    dv.texels = sc->texels.as<float>(); dv.weightLut = sc->weightLut.as<float>();
    dv.instances = sc->instances.as<DevInstance>(); dv.nInstances = d->n_instances;
    dv.topEntry = L.topEntry.empty() ? nullptr : sc->topEntry.as<float4>(); dv.nTopPrims = (uint32_t)L.topEntry.size();
    dv.topEntryWide = L.topEntryWide.empty() ? nullptr : sc->topEntryWide.as<float4>();
    dv.lightFunc = sc->lightFunc.as<float>(); dv.lightCdf = sc->lightCdf.as<float>(); dv.lightFuncInt = L.funcInt;
    dv.deepStack = sc->deepStack.as<uint2>();
    dv.perms = sc->perms.as<uint16_t>(); dv.primes = sc->primes.as<int32_t>(); dv.primeSums = sc->primeSums.as<int32_t>();
    dv.primeMagic = sc->primeMagic.as<uint64_t>();
    dv.worldRadius = L.worldRadius;
    dv.spatial = 0; dv.voxFunc = dv.voxCdf = dv.voxFuncInt = nullptr;
    dv.voxSlot = nullptr; dv.voxRequest = nullptr; dv.voxRequestCount = nullptr;
    for (int a = 0; a < 3; ++a) { dv.voxN[a] = L.voxN[a]; dv.wbMin[a] = L.wbMin[a]; dv.wbMax[a] = L.wbMax[a]; }
    if (L.lightStrategy == 2) {
        // SpatialLightDistribution (core/lightdistrib.cpp:95-120, maxVoxels = 64) over the voxel grid of the layout.  The reference
        // fills a voxel's distribution when a vertex first falls into it; a voxel's distribution being a pure function of the voxel,
        // here every voxel is computed now, on the device (k_voxel_contrib / k_voxel_dist).
        const uint64_t nVox = (uint64_t)dv.voxN[0] * (uint64_t)dv.voxN[1] * (uint64_t)dv.voxN[2];
        // The table of every voxel (2 * nLights + 2 floats each) is computed now when it is small: a lookup is then a plain read.  With
        // many lights (every triangle of an emissive mesh is one, core/api.cpp:1609-1636) it is not — 64^3 voxels x 500 lights is
        // already 1 GiB — and the reference never builds it either: it fills a voxel when a vertex first falls into it
        // (core/lightdistrib.cpp:149-229).  Same here then, per batch: a bounded pool of rows, a voxel -> row map, and the
        // bounce loop computes the rows its vertices asked for (RunBatch).  HPRT_VOXEL_DENSE_MAX_MB moves the switch (tests: 0).
        const uint64_t denseMaxFloats = [] { const char *e = getenv("HPRT_VOXEL_DENSE_MAX_MB"); return e ? (uint64_t)atoll(e) * (1ull << 18) : (1ull << 28); }();      // (read per scene: tests switch it)
        const uint64_t rowFloats = 2ull * d->n_lights + 2ull;
        const bool dense = nVox * rowFloats <= denseMaxFloats;
        uint64_t rows = nVox;
        if (!dense) {
            // pool: up to 4 GiB of rows (HPRT_VOXEL_POOL_MB), never more than there are voxels, at least one
            const uint64_t poolFloats = [] { const char *e = getenv("HPRT_VOXEL_POOL_MB"); return (e ? (uint64_t)atoll(e) : 4096ull) * (1ull << 18); }();
            rows = std::max<uint64_t>(1, std::min<uint64_t>(nVox, poolFloats / rowFloats));
        }
        HIP_TRY(sc->voxFunc.alloc(rows * d->n_lights * sizeof(float)));
        HIP_TRY(sc->voxCdf.alloc(rows * (d->n_lights + 1ull) * sizeof(float)));
        HIP_TRY(sc->voxFuncInt.alloc(rows * sizeof(float)));
        std::vector<float> ri(5 * 128);
        VoxelSamplePoints(ri.data());
        HIP_TRY(upload(sc->voxRi, ri));
        dv.spatial = 1;
        dv.voxFunc = sc->voxFunc.as<float>(); dv.voxCdf = sc->voxCdf.as<float>(); dv.voxFuncInt = sc->voxFuncInt.as<float>();
        sc->nVoxels = (uint32_t)nVox; sc->voxRows = (uint32_t)rows; sc->voxRowsUsed = 0;
        if (dense) LaunchVoxelDistributions(nullptr, dv, sc->voxRi.as<float>(), (uint32_t)nVox, sc->voxFunc.as<float>(), sc->voxCdf.as<float>(), sc->voxFuncInt.as<float>());
        else {
            HIP_TRY(sc->voxSlot.alloc(nVox * sizeof(int32_t)));
            HIP_TRY(hipMemset(sc->voxSlot.p, 0xff, nVox * sizeof(int32_t)));      // VOX_EMPTY
            HIP_TRY(sc->voxRequest.alloc(nVox * sizeof(uint32_t)));
            HIP_TRY(sc->voxRequestCount.alloc(256));
            HIP_TRY(hipMemset(sc->voxRequestCount.p, 0, 256));
            dv.voxSlot = sc->voxSlot.as<int32_t>(); dv.voxRequest = sc->voxRequest.as<uint32_t>(); dv.voxRequestCount = sc->voxRequestCount.as<uint32_t>();
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
    }
    HIP_TRY(hipHostMalloc((void **)&sc->hostCounts, (4096 + 256) * sizeof(uint32_t)));
    *out = sc.release();
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }

// Diagnostics hook (not part of include/hprt.h): 1 when plain renders of this scene take the leaf-exact wide walk (k_walk4), else 0: the
// binary walk, or an attached tree's walk (callers test the value for truth: "is it k_walk4")
__attribute__((visibility("default"))) int hprt_debug_scene_walk(HprtScene *s) { return s && s->walk == HprtScene::Walk::Bvh && hprt::WideWalkInUse(s->dev) ? 1 : 0; }
// Diagnostics hook (not part of include/hprt.h; tests/test_gpu_shade_chain.py): on != 0 starts counting (from zero) the vertices deferred to the
// generic bin and the vertices shaded again by a retry pass; out2, if given, receives {deferred, retried} so far.
__attribute__((visibility("default"))) int hprt_debug_shade_counts(HprtScene *s, int on, uint64_t *out2) {
    if (!s) return HPRT_E_INVALID;
    if (out2) { out2[0] = s->shadeDeferred; out2[1] = s->shadeRetried; }
    if (on && !s->shadeCountsOn) s->shadeDeferred = s->shadeRetried = s->shadeSpeculated = s->shadeRepaired = s->shadeFull = 0;
    s->shadeCountsOn = on != 0;
    return HPRT_OK;
}
// Diagnostics hook (not part of include/hprt.h; tests/test_gpu_speculated_light.py): the sums, since hprt_debug_shade_counts switched counting
// on, of the vertices whose light sample k_shade added at once, of those k_repair then set back (their shadow ray was blocked), and of
// the full vertices (pending streams + k_resolve)
__attribute__((visibility("default"))) int hprt_debug_speculated_counts(HprtScene *s, uint64_t *out3) {
    if (!s || !out3) return HPRT_E_INVALID;
    out3[0] = s->shadeSpeculated; out3[1] = s->shadeRepaired; out3[2] = s->shadeFull;
    return HPRT_OK;
}
// HPRT_SPECULATE_LIGHT=0 in the environment, or hprt_debug_speculate_light(0) at run time (diagnostics hook, not part of include/hprt.h):
// renders keep the full path for every vertex — all pending terms through k_resolve (A/B runs, tests).  Returns the setting before.
static int g_speculateLight = -1;
static bool SpeculateLightEnabled() {
    static const bool fromEnv = [] { const char *e = getenv("HPRT_SPECULATE_LIGHT"); return !(e && atoi(e) == 0); }();
    return g_speculateLight < 0 ? fromEnv : g_speculateLight != 0;
}
__attribute__((visibility("default"))) int hprt_debug_speculate_light(int on) { const int was = SpeculateLightEnabled() ? 1 : 0; g_speculateLight = on; return was; }
// HPRT_FOLD_REPAIR=0 in the environment, or hprt_debug_fold_repair(0) at run time (diagnostics hook, not part of include/hprt.h): every
// speculated vertex's shadow ray goes through k_repair and no path segment is marked, as before the repair was folded into the next
// bounce's readers (A/B runs, tests).  Returns the setting before.
static int g_foldRepair = -1;
static bool FoldRepairEnabled() {
    static const bool fromEnv = [] { const char *e = getenv("HPRT_FOLD_REPAIR"); return !(e && atoi(e) == 0); }();
    return g_foldRepair < 0 ? fromEnv : g_foldRepair != 0;
}
__attribute__((visibility("default"))) int hprt_debug_fold_repair(int on) { const int was = FoldRepairEnabled() ? 1 : 0; g_foldRepair = on; return was; }
__attribute__((visibility("default"))) int hprt_debug_poison_workspace(HprtScene *s, int byte) { if (!s) return HPRT_E_INVALID; s->poisonByte = byte < 0 ? -1 : (byte & 255); return HPRT_OK; }
// Diagnostics hook (not part of include/hprt.h): the first batch of the next hprt_render copies the rays that bounce `bounce` queues
// (kind 0: the path segments entering bounce + 1, 1: its shadow rays, 2: its BSDF-sampled light rays) into d_out7 ([7][cap] planes:
// ox oy oz dx dy dz tmax); hprt_debug_captured returns how many.  d_out7 == NULL switches it off.
__attribute__((visibility("default"))) int hprt_debug_capture_rays(HprtScene *s, int bounce, int kind, float *d_out7, size_t cap) {
    if (!s || kind < 0 || kind > 2 || cap > 0x7fffffffull) return HPRT_E_INVALID;
    s->capture.bounce = bounce; s->capture.kind = kind; s->capture.out7 = d_out7; s->capture.cap = cap; s->capture.n = 0;
    return HPRT_OK;
}
static int ApiStreams(HprtScene *s, size_t n, RayStream *rays, HitStream *hits);
// The walks that count their kd interior nodes apart (kdShare, pixelKdLocal / pixelKdFilm)
static bool CountsKdShare(const HprtScene *s) {
    return s->walk == HprtScene::Walk::RbspKd || s->walk == HprtScene::Walk::BspPaperKd || s->walk == HprtScene::Walk::RbspKdInst ||
           s->walk == HprtScene::Walk::BspPaperKdInst;
}
// Every trace of a scene: the walk of the attached tree (AttachTree below), else the BVH walks (LaunchTrace)
static void Trace(HprtScene *s, hipStream_t st, bool anyHit, bool count, const uint32_t *queue, const uint32_t *countPtr, uint32_t countImm,
                  uint32_t gridItems, const RayStream &rays, const HitStream &hits, uint8_t *occ, DevCounters *counters, uint32_t *workCounter,
                  uint4 *rayStats = nullptr) {
    switch (s->walk) {
    case HprtScene::Walk::Kd: LaunchKdTrace(st, s->dev, s->kd, anyHit, count, queue, countPtr, countImm, gridItems, rays, hits, occ, counters, workCounter, rayStats); break;
    case HprtScene::Walk::Rbsp: LaunchRbspTrace(st, s->dev, s->rbsp, anyHit, count, queue, countPtr, countImm, gridItems, rays, hits, occ, counters, workCounter, rayStats); break;
    case HprtScene::Walk::RbspKd:
        LaunchRbspKdTrace(st, s->dev, DevRbspKd{s->rbsp, s->kdShare.as<unsigned long long>()}, anyHit, count, queue, countPtr, countImm, gridItems, rays,
                          hits, occ, counters, workCounter, rayStats);
        break;
    case HprtScene::Walk::BspPaper:
        LaunchBspPaperTrace(st, s->dev, s->bsppaper, anyHit, count, queue, countPtr, countImm, gridItems, rays, hits, occ, counters, workCounter, rayStats);
        break;
    case HprtScene::Walk::BspPaperKd:
        LaunchBspPaperKdTrace(st, s->dev, DevBspPaperKd{s->bsppaper, s->kdShare.as<unsigned long long>()}, anyHit, count, queue, countPtr, countImm,
                              gridItems, rays, hits, occ, counters, workCounter, rayStats);
        break;
    case HprtScene::Walk::KdInst:
        LaunchKdInstTrace(st, s->dev, s->kdinst, anyHit, count, queue, countPtr, countImm, gridItems, rays, hits, occ, counters, workCounter, rayStats);
        break;
    case HprtScene::Walk::RbspInst:
    case HprtScene::Walk::RbspKdInst:
        LaunchRbspInstTrace(st, s->dev, s->rbspinst, s->walk == HprtScene::Walk::RbspKdInst, anyHit, count, queue, countPtr, countImm, gridItems, rays, hits, occ,
                            counters, workCounter, rayStats);
        break;
    case HprtScene::Walk::BspPaperInst:
    case HprtScene::Walk::BspPaperKdInst:
        LaunchBspPaperInstTrace(st, s->dev, s->bsppaperinst, s->walk == HprtScene::Walk::BspPaperKdInst, anyHit, count, queue, countPtr, countImm, gridItems, rays,
                                hits, occ, counters, workCounter, rayStats);
        break;
    case HprtScene::Walk::Bvh: LaunchTrace(st, s->dev, anyHit, count, queue, countPtr, countImm, gridItems, rays, hits, occ, counters, workCounter, rayStats); break;
    }
}
// The shadow rays of a plain render go to k_shadow_grid: the scene has a grid (eligibility: scene_layout.cpp, LayoutShadowGrid), still
// walks its BVH and takes the leaf-exact walk, whose leaf boxes the grid kernel tests with.  hprt_debug_shadow_grid(0) keeps the walk.
static int g_shadowGrid = -1;
static bool GridInUse(const HprtScene *s) {
    // (a phase-profile render keeps the walk: its any-hit records per ray are k_walk4's, and the grid kernels have no profile variant)
    return s->gridKind != GridKind::None && g_shadowGrid != 0 && s->walk == HprtScene::Walk::Bvh && hprt::WideWalkInUse(s->dev) && !hprt::TraceProfileInUse();
}
// The scene's grid kernel — k_shadow_grid for a point light's grid, k_distant_grid (distant_grid.h) for a distant light's —
// over the rays of a queue
static void LaunchGrid(const HprtScene *s, hipStream_t st, const uint32_t *queue, uint32_t n, const RayStream &rays, uint8_t *occ, uint32_t *workCounter) {
    const DevDistantGrid &g = s->grid;
    if (s->gridKind == GridKind::Point) LaunchShadowGrid(st, s->dev, DevShadowGrid{g.image, g.imageBytes, g.recordsAt, g.nNear, g.R}, queue, nullptr, n, n, rays, occ, workCounter);
    else LaunchDistantGrid(st, s->dev, g, queue, nullptr, n, n, rays, occ, workCounter);
}
// What the hooks of one kind see of a scene: its grid if it is of that kind, else none, all zeros
struct GridOfKind {
    bool has = false; DevDistantGrid g{}; HprtScene::GridInfo info;
    GridOfKind(const HprtScene *s, GridKind k) { if (s->gridKind == k) { has = true; g = s->grid; info = s->gridInfo; } }
    double meanList(double faces) const { return has ? (double)(info.nEntries - g.nNear) / (faces * g.R * g.R) : 0.0; }
};
// the image a grid kernel reads of this scene (shadow_grid.h, ShadowGridImage), copied back from the device: words2 = {block words,
// record words, the padding included}; each array is written when it fits its capacity in words.
static int GridImageRead(HprtScene *s, GridKind k, const char *badArg, const char *noGrid, size_t words2[2], uint32_t *blocks, size_t block_cap, uint32_t *records, size_t record_cap) try {
    if (!s || !words2) return SetError(HPRT_E_INVALID, badArg);
    if (s->gridKind != k) return SetError(HPRT_E_UNSUPPORTED, noGrid);
    HIP_TRY(hipSetDevice(s->device));
    const DevDistantGrid &g = s->grid;
    words2[0] = g.recordsAt / sizeof(uint32_t); words2[1] = (g.imageBytes - g.recordsAt) / sizeof(uint32_t);
    if (blocks && block_cap >= words2[0]) HIP_TRY(hipMemcpy(blocks, g.image, words2[0] * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (records && record_cap >= words2[1]) HIP_TRY(hipMemcpy(records, g.image + words2[0], words2[1] * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
// the scene's grid kernel on the n rays of d_rays7 ([7][n] planes, as hprt_occluded_device takes them), every one formed as a render
// forms the shadow rays of the scene's light (a point light: d = light - o in float); ms, if given, receives the kernel's time.
static int GridOccluded(HprtScene *s, GridKind k, const char *badArg, const char *noGrid, size_t n, const float *d_rays7, uint8_t *d_occ, float *ms) try {
    if (!s || !d_rays7 || !d_occ || n == 0 || n > 0x7ffffff0ull) return SetError(HPRT_E_INVALID, badArg);
    if (s->gridKind != k) return SetError(HPRT_E_UNSUPPORTED, noGrid);
    HIP_TRY(hipSetDevice(s->device));
    SceneCall call(s, nullptr);
    RayStream rays; HitStream hits;
    if (int rc = ApiStreams(s, n, &rays, &hits)) return rc;
    struct Events { hipEvent_t e[2] = {nullptr, nullptr}; ~Events() { for (auto x : e) if (x) (void)hipEventDestroy(x); } } ev;
    for (auto &x : ev.e) HIP_TRY(hipEventCreate(&x));
    LaunchPackRays(nullptr, d_rays7, (uint32_t)n, rays);
    HIP_TRY(hipEventRecord(ev.e[0], nullptr));
    LaunchGrid(s, nullptr, nullptr, (uint32_t)n, rays, d_occ, s->workCounter.as<uint32_t>());
    HIP_TRY(hipEventRecord(ev.e[1], nullptr));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    if (ms) HIP_TRY(hipEventElapsedTime(ms, ev.e[0], ev.e[1]));
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
// Diagnostics hooks (not part of include/hprt.h; tests/test_gpu_shadow_grid.py, tools/shadow_grid_replay.py).
// hprt_debug_shadow_grid: on = 0 sends the shadow rays of later renders through the walk again, 1 through the grid where a scene has
// one, -1 back to the default; returns the setting before.
__attribute__((visibility("default"))) int hprt_debug_shadow_grid(int on) { const int was = g_shadowGrid; g_shadowGrid = on; return was; }
// hprt_debug_shadow_grid_info: out = {eligible, R, entries, near-list length, bytes of the device image, build and pack seconds, longest list, mean list, light x y z,
// launches of k_shadow_grid by this scene's renders so far}
__attribute__((visibility("default"))) int hprt_debug_shadow_grid_info(HprtScene *s, double out[12]) {
    if (!s || !out) return HPRT_E_INVALID;
    const GridOfKind v(s, GridKind::Point);
    out[0] = v.has ? 1 : 0; out[1] = v.g.R; out[2] = (double)v.info.nEntries; out[3] = v.g.nNear; out[4] = (double)v.info.bytes;
    out[5] = v.info.buildSeconds + v.info.packSeconds; out[6] = v.info.longest; out[7] = v.meanList(6.0);
    for (int a = 0; a < 3; ++a) out[8 + a] = v.info.light[a];
    out[11] = (double)v.info.renderLaunches;
    return HPRT_OK;
}
__attribute__((visibility("default"))) int hprt_debug_shadow_grid_image_read(HprtScene *s, size_t words2[2], uint32_t *blocks, size_t block_cap, uint32_t *records, size_t record_cap) {
    return GridImageRead(s, GridKind::Point, "hprt_debug_shadow_grid_image_read: bad argument", "hprt_debug_shadow_grid_image_read: the scene has no shadow grid", words2, blocks, block_cap, records, record_cap);
}
__attribute__((visibility("default"))) int hprt_debug_shadow_grid_occluded(HprtScene *s, size_t n, const float *d_rays7, uint8_t *d_occ, float *ms) {
    return GridOccluded(s, GridKind::Point, "hprt_debug_shadow_grid_occluded: bad argument", "hprt_debug_shadow_grid_occluded: the scene has no shadow grid", n, d_rays7, d_occ, ms);
}
// The distant light's grid (not part of include/hprt.h; tests/test_gpu_distant_grid.py, tools/distant_grid_replay.py).
// hprt_debug_distant_grid_info: out = {has a grid, R, entries, near-list length, bytes of the device image, build seconds, pack seconds,
// longest list, mean list, w x y z, U x y z, V x y z, launches of k_distant_grid by this scene's renders so far, eps}
__attribute__((visibility("default"))) int hprt_debug_distant_grid_info(HprtScene *s, double out[20]) {
    if (!s || !out) return HPRT_E_INVALID;
    const GridOfKind v(s, GridKind::Distant);
    out[0] = v.has ? 1 : 0; out[1] = v.g.R; out[2] = (double)v.info.nEntries; out[3] = v.g.nNear; out[4] = (double)v.info.bytes;
    out[5] = v.info.buildSeconds; out[6] = v.info.packSeconds; out[7] = v.info.longest; out[8] = v.meanList(1.0);
    for (int a = 0; a < 3; ++a) { out[9 + a] = v.g.f.W[a]; out[12 + a] = v.g.f.U[a]; out[15 + a] = v.g.f.V[a]; }
    out[18] = (double)v.info.renderLaunches; out[19] = v.info.eps;
    return HPRT_OK;
}
__attribute__((visibility("default"))) int hprt_debug_distant_grid_image_read(HprtScene *s, size_t words2[2], uint32_t *blocks, size_t block_cap, uint32_t *records, size_t record_cap) {
    return GridImageRead(s, GridKind::Distant, "hprt_debug_distant_grid_image_read: bad argument", "hprt_debug_distant_grid_image_read: the scene has no distant grid", words2, blocks, block_cap, records, record_cap);
}
__attribute__((visibility("default"))) int hprt_debug_distant_grid_occluded(HprtScene *s, size_t n, const float *d_rays7, uint8_t *d_occ, float *ms) {
    return GridOccluded(s, GridKind::Distant, "hprt_debug_distant_grid_occluded: bad argument", "hprt_debug_distant_grid_occluded: the scene has no distant grid", n, d_rays7, d_occ, ms);
}
// Diagnostics (tools/sort_experiment.py): what consuming rays through a PERMUTED index queue costs.  The n rays of d_rays7 stay where
// they are; d_queue lists them in the order to be traced.  ms[0]: a streaming pass that gathers the rays through the queue into
// [7][n] planes at d_scratch7 (the physical permutation a sort would have to do), ms[1]: the scene's walk reading the rays through the queue.
__attribute__((visibility("default"))) int hprt_debug_trace_queued(HprtScene *s, size_t n, const float *d_rays7, const uint32_t *d_queue, int anyHit,
                                                                    float *d_scratch7, float ms[2]) try {
    if (!s || !d_rays7 || !d_queue || !d_scratch7 || !ms || n == 0 || n > 0x7ffffff0ull) return SetError(HPRT_E_INVALID, "hprt_debug_trace_queued: bad argument");
    HIP_TRY(hipSetDevice(s->device));
    SceneCall call(s, nullptr);
    RayStream rays; HitStream hits;
    if (int rc = ApiStreams(s, n, &rays, &hits)) return rc;
    DevBuf occ; HIP_TRY(occ.alloc(n));
    hipEvent_t e[3];
    for (auto &x : e) HIP_TRY(hipEventCreate(&x));
    LaunchPackRays(nullptr, d_rays7, (uint32_t)n, rays);
    HIP_TRY(hipEventRecord(e[0], nullptr));
    LaunchCaptureRays(nullptr, d_queue, (uint32_t)n, rays, d_scratch7, (uint32_t)n);
    HIP_TRY(hipEventRecord(e[1], nullptr));
    HitStream none; none.a = nullptr; none.b = nullptr;
    Trace(s, nullptr, anyHit != 0, false, d_queue, nullptr, (uint32_t)n, (uint32_t)n, rays, anyHit ? none : hits, anyHit ? occ.as<uint8_t>() : nullptr, nullptr, s->workCounter.as<uint32_t>());
    HIP_TRY(hipEventRecord(e[2], nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipEventElapsedTime(&ms[0], e[0], e[1])); HIP_TRY(hipEventElapsedTime(&ms[1], e[1], e[2]));
    for (auto &x : e) (void)hipEventDestroy(x);
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
__attribute__((visibility("default"))) long long hprt_debug_captured(HprtScene *s) { return s ? (long long)s->capture.n : -1; }
// Measurement hook (not part of include/hprt.h): HBM stream bandwidth of this box, a float4 copy of `bytes` bytes (src and dst far
// larger than the 256 MB Infinity Cache), timed with HIP events over `iters` launches after one warm-up; GB/s count read + write.
__attribute__((visibility("default"))) int hprt_debug_stream_copy(int device, size_t bytes, int iters, double *best_gbs, double *mean_gbs) try {
    if (!best_gbs || !mean_gbs || iters < 1 || iters > 1000 || bytes < (1u << 20) || bytes > (64ull << 30)) return SetError(HPRT_E_INVALID, "hprt_debug_stream_copy: bad argument");
    int dev = 0;
    if (int rc = CheckDevice(device, &dev)) return rc;
    HIP_TRY(hipSetDevice(dev));
    DevBuf a, b;
    HIP_TRY(a.alloc(bytes)); HIP_TRY(b.alloc(bytes));
    HIP_TRY(hipMemset(a.p, 1, bytes)); HIP_TRY(hipMemset(b.p, 2, bytes));
    const size_t n = bytes / 16;
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1));
    LaunchStreamCopy(nullptr, a.as<float4>(), b.as<float4>(), n);
    HIP_TRY(hipDeviceSynchronize());
    double best = 0, sum = 0;
    for (int i = 0; i < iters; ++i) {
        HIP_TRY(hipEventRecord(e0, nullptr));
        LaunchStreamCopy(nullptr, a.as<float4>(), b.as<float4>(), n);
        HIP_TRY(hipEventRecord(e1, nullptr));
        HIP_TRY(hipEventSynchronize(e1));
        float ms = 0; HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        const double g = 2.0 * (double)(n * 16) / ((double)ms * 1e-3) / 1e9;
        best = std::max(best, g); sum += g;
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    *best_gbs = best; *mean_gbs = sum / iters;
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
// Diagnostics hook (not part of include/hprt.h): rate at which the device serves dependent per-lane gathers of 64-byte records
// over a BVH-like pick from a table of 2^log2_records records (kernels.hip, k_gather_probe) — the measured ceiling bench.py holds
// k_trace's record rate against.  Out: records per second (1e9), best and mean of `launches` timed launches.
__attribute__((visibility("default"))) int hprt_debug_gather_probe(int device, int log2_records, int iters_per_lane, int launches, double *best_grecords_s, double *mean_grecords_s) try {
    if (!best_grecords_s || !mean_grecords_s || log2_records < 8 || log2_records > 26 || iters_per_lane < 1 || iters_per_lane > 100000 || launches < 1 || launches > 100)
        return SetError(HPRT_E_INVALID, "hprt_debug_gather_probe: bad argument");
    int dev = 0;
    if (int rc = CheckDevice(device, &dev)) return rc;
    HIP_TRY(hipSetDevice(dev));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, dev));
    const uint32_t blocks = (uint32_t)prop.multiProcessorCount * 6u * 4u;
    DevBuf table, sink;
    const size_t bytes = (size_t)64 << log2_records;
    HIP_TRY(table.alloc(bytes)); HIP_TRY(sink.alloc(16));
    HIP_TRY(hipMemset(table.p, 0x5b, bytes));
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1));
    LaunchGatherProbe(nullptr, table.as<uint4>(), (uint32_t)log2_records, std::max(1, iters_per_lane / 10), blocks, sink.as<uint32_t>());
    HIP_TRY(hipDeviceSynchronize());
    double best = 0, sum = 0;
    for (int i = 0; i < launches; ++i) {
        HIP_TRY(hipEventRecord(e0, nullptr));
        LaunchGatherProbe(nullptr, table.as<uint4>(), (uint32_t)log2_records, iters_per_lane, blocks, sink.as<uint32_t>());
        HIP_TRY(hipEventRecord(e1, nullptr));
        HIP_TRY(hipEventSynchronize(e1));
        float ms = 0; HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        const double g = (double)blocks * 256.0 * (double)iters_per_lane / ((double)ms * 1e-3) / 1e9;
        best = std::max(best, g); sum += g;
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    *best_grecords_s = best; *mean_grecords_s = sum / launches;
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }

// Diagnostics hook (not part of include/hprt.h): the restated libm functions of hprt_math.h evaluated ON THE DEVICE over host
// arrays, so that a test can hold them against the oracle's (which equal glibc's, tests/test_oracle_pins.py) directly rather
// than through renders.  fn 0: sinf / cosf of x -> out0 / out1; 1: acosf(x) -> out0; 2: atan2f(y, x) -> out0; 3: logf(x) -> out0;
// 4: double sin / cos of (double)x -> out0 / out1.  Outputs are doubles (a float result converts exactly).
__global__ void k_debug_math(int fn, const float *x, const float *y, size_t n, double *o0, double *o1) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double a = 0, b = 0;
    if (fn == 0) { float s, c; det_sincosf(x[i], &s, &c); a = (double)s; b = (double)c; }
    else if (fn == 1) a = (double)det_acosf(x[i]);
    else if (fn == 2) a = (double)det_atan2f(y[i], x[i]);
    else if (fn == 3) a = (double)det_logf(x[i]);
    else det_sincos_glibc_d((double)x[i], &a, &b);
    o0[i] = a; o1[i] = b;
}
__attribute__((visibility("default"))) int hprt_debug_device_math(int device, int fn, const float *x, const float *y, size_t n, double *out0, double *out1) try {
    if (fn < 0 || fn > 4 || !x || !y || !out0 || !out1 || n == 0 || n > ((size_t)1 << 28)) return SetError(HPRT_E_INVALID, "hprt_debug_device_math: bad argument");
    HIP_TRY(hipSetDevice(device));
    float *dx = nullptr, *dy = nullptr; double *d0 = nullptr, *d1 = nullptr;
    auto release = [&]() { (void)hipFree(dx); (void)hipFree(dy); (void)hipFree(d0); (void)hipFree(d1); };
    hipError_t e = hipMalloc((void **)&dx, n * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&dy, n * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&d0, n * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&d1, n * 8);
    if (e == hipSuccess) e = hipMemcpy(dx, x, n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dy, y, n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        k_debug_math<<<dim3((unsigned)((n + 255) / 256)), dim3(256)>>>(fn, dx, dy, n, d0, d1);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out0, d0, n * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out1, d1, n * 8, hipMemcpyDeviceToHost);
    release();
    if (e != hipSuccess) return SetError(HPRT_E_DEVICE, std::string("hprt_debug_device_math: ") + hipGetErrorString(e));
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }

// A host tree as AttachTree takes it: GenericBSP's node array over M directions (bsp_tree.h) with creation-order primitive numbers,
// its bounds, its direction table (none for the kd-tree), the deepest tree its walk takes and the builder's structural check, and
// for a tree whose nodes carry their own split axis (bsppaper, bsppaperkd) those axes, 3 floats per node.  flagBits / leafTag: a
// node layout that is not GenericBSP's over M directions (bsppaperkd: 3 flag bits, leaves tagged 3); 0 flagBits: derived from M
struct TreeView {
    const char *what;                                       // the tree's name in messages
    const std::vector<BspNode> &nodes; const std::vector<uint32_t> &primIndices; uint32_t nPrims; const float *bounds;
    uint32_t M; const std::vector<float> *dirs; uint32_t todoMax;
    std::function<const char *(uint32_t *depth)> check;     // CheckKdTree, CheckRbspTree, CheckBspPaperTree
    const std::vector<float> *axes = nullptr;
    uint32_t flagBits = 0, leafTag = 0;
};
// MakeAccelerator (core/api.cpp:790-831) for the trees the host builds: the tree is checked, its creation-order primitive numbers are
// mapped to the scene's ordered indices (the inverse of prim_order), and from now on every trace of the scene takes `walk` over it
// (Trace above).  Until the upload has succeeded the scene walks its BVH: a failed attach never leaves a half-replaced tree behind.
// The steps every attach shares (AttachTree, AttachTwoLevel).
// InvertOrder: a prim_order (ordered position -> creation number) turned round, with the aggregate's first ordered index added.
static std::vector<uint32_t> InvertOrder(const std::vector<uint32_t> &order, uint32_t primBase) {
    std::vector<uint32_t> toOrdered(order.size());
    for (uint32_t i = 0; i < (uint32_t)order.size(); ++i) toOrdered[order[i]] = primBase + i;
    return toOrdered;
}
// AppendTree: one host tree behind whatever the upload arrays hold already — its creation-order primitive numbers mapped to ordered
// indices (one-primitive leaves and primitiveIndices), and, where trees share the arrays, aboveChild and primitiveIndicesOffset
// rebased (by nothing for the first tree).  off / mask / leafTag: the node layout.  Returns the tree's root.
static uint32_t AppendTree(const std::vector<BspNode> &tree, const std::vector<uint32_t> &primIndices, const std::vector<uint32_t> &toOrdered,
                           uint32_t off, uint32_t mask, uint32_t leafTag, std::vector<uint2> *nodes, std::vector<uint32_t> *prims) {
    const uint32_t nodeBase = (uint32_t)nodes->size(), idxBase = (uint32_t)prims->size();
    for (const BspNode &nd : tree) {
        const uint32_t high = nd.b >> off;
        if ((nd.b & mask) != leafTag) nodes->push_back(make_uint2(nd.a, (nd.b & mask) | ((high + nodeBase) << off)));
        else nodes->push_back(make_uint2(high == 1u ? toOrdered[nd.a] : high == 0u ? nd.a : nd.a + idxBase, nd.b));
    }
    for (uint32_t p : primIndices) prims->push_back(toOrdered[p]);
    return nodeBase;
}
// UploadTree: the arrays replace the attached tree's.  From here until the caller sets its walk the scene walks its BVH: a failed
// upload never leaves a half-replaced tree behind (it does leave the BVH, not the tree that was attached before).
static int UploadTree(HprtScene *s, const std::vector<uint2> &nodes, const std::vector<uint32_t> &prims) {
    HIP_TRY(hipDeviceSynchronize());      // a render or trace of the old tree may still be running
    s->walk = HprtScene::Walk::Bvh;
    HIP_TRY(upload(s->treeNodes, nodes));
    HIP_TRY(upload(s->treePrims, prims));
    return HPRT_OK;
}
// FillTree: the fields every walk's descriptor shares (DevKd, DevRbsp, DevBspPaper, DevKdInst, DevRbspInst)
extern "C++" template <class Dev> static void FillTree(Dev &d, const HprtScene *s, size_t nNodes, size_t nPrims, const float *bounds, uint32_t depth) {
    d.nodes = s->treeNodes.as<uint2>(); d.nNodes = (uint32_t)nNodes;
    d.primIdx = s->treePrims.as<uint32_t>(); d.nPrimIdx = (uint32_t)nPrims;
    for (int a = 0; a < 3; ++a) { d.lo[a] = bounds[a]; d.hi[a] = bounds[3 + a]; }
    d.depth = depth;
}
// ResetKdShare: the kd counter pair of a walk that counts its kd interior nodes apart (CountsKdShare), allocated and zeroed
static int ResetKdShare(HprtScene *s) {
    HIP_TRY(s->kdShare.alloc(2 * sizeof(unsigned long long)));
    HIP_TRY(hipMemset(s->kdShare.p, 0, 2 * sizeof(unsigned long long)));
    return HPRT_OK;
}
static int AttachTree(HprtScene *s, HprtScene::Walk walk, const TreeView &t) {
    const std::string what = t.what;
    if (s->instanced) return SetError(HPRT_E_UNSUPPORTED, what + "s over object instances are not supported: the scene keeps its BVH");
    HIP_TRY(hipSetDevice(s->device));
    SceneCall call(s, nullptr);
    const uint32_t nTop = (uint32_t)s->topOrder.size();
    if (t.nPrims != nTop)
        return SetError(HPRT_E_INVALID, "the " + what + " holds " + std::to_string(t.nPrims) + " primitives, the scene " + std::to_string(nTop));
    uint32_t depth = 0;
    const char *bad = t.check(&depth);
    if (*bad) return SetError(HPRT_E_INVALID, "malformed " + what + ": " + bad);
    if (depth > t.todoMax)
        return SetError(HPRT_E_UNSUPPORTED, what + " of depth " + std::to_string(depth) + " is deeper than the walk's todo list (" + std::to_string(t.todoMax) + ")");
    const uint32_t off = t.flagBits ? t.flagBits : RbspBitOffset(t.M), mask = t.flagBits ? (1u << t.flagBits) - 1u : RbspBitMask(t.M);
    const uint32_t leafTag = t.flagBits ? t.leafTag : t.M;
    std::vector<uint2> nodes; std::vector<uint32_t> prims;
    AppendTree(t.nodes, t.primIndices, InvertOrder(s->topOrder, 0u), off, mask, leafTag, &nodes, &prims);
    if (int rc = UploadTree(s, nodes, prims)) return rc;
    if (t.axes) {       // 16 bytes per node (hipMalloc aligns far beyond), leaves zero as the builder holds them
        std::vector<float4> axes(t.nodes.size());
        for (size_t k = 0; k < axes.size(); ++k) axes[k] = make_float4((*t.axes)[3 * k], (*t.axes)[3 * k + 1], (*t.axes)[3 * k + 2], 0.f);
        HIP_TRY(upload(s->treeAxes, axes));
    }
    if (walk == HprtScene::Walk::RbspKd || walk == HprtScene::Walk::BspPaperKd)
        if (int rc = ResetKdShare(s)) return rc;
    auto fill = [&](auto &d) { FillTree(d, s, nodes.size(), prims.size(), t.bounds, depth); };
    if (walk == HprtScene::Walk::Kd) fill(s->kd);
    else if (walk == HprtScene::Walk::BspPaper || walk == HprtScene::Walk::BspPaperKd) {
        s->bsppaper = DevBspPaper{};
        fill(s->bsppaper);
        s->bsppaper.axes = s->treeAxes.as<float4>();
    } else {
        s->rbsp = DevRbsp{};
        fill(s->rbsp);
        s->rbsp.M = t.M; s->rbsp.off = off; s->rbsp.mask = mask;
        for (uint32_t k = 0; k < 3 * t.M; ++k) s->rbsp.dirs[k] = (*t.dirs)[k];
    }
    s->walk = walk;
    return HPRT_OK;
}

int hprt_scene_attach_kdtree(HprtScene *s, const HprtKdTree *t) try {
    if (!s || !t) return SetError(HPRT_E_INVALID, "hprt_scene_attach_kdtree: null argument");
    const KdTree &kt = t->tree;
    return AttachTree(s, HprtScene::Walk::Kd, {"kd-tree", kt.nodes, kt.primIndices, kt.nPrims, kt.bounds, 3u, nullptr, (uint32_t)KD_TODO_MAX,
                                               [&](uint32_t *depth) { return CheckKdTree(kt, depth); }});
} catch (...) { return hprt::HandleException(); }
// An RBSP tree (either cost model) for the RBSP walk or the rbspkd walk with its kd counter pair; `what` names it in messages
static int AttachRbsp(HprtScene *s, HprtScene::Walk walk, const char *what, const RbspTree &rt) {
    return AttachTree(s, walk, {what, rt.nodes, rt.primIndices, rt.nPrims, rt.bounds, rt.M, &rt.directions, (uint32_t)RBSP_TODO_MAX,
                                [&](uint32_t *depth) { return CheckRbspTree(rt, depth); }});
}
int hprt_scene_attach_rbsp(HprtScene *s, const HprtRbsp *t) try {
    if (!s || !t) return SetError(HPRT_E_INVALID, "hprt_scene_attach_rbsp: null argument");
    return AttachRbsp(s, HprtScene::Walk::Rbsp, "RBSP tree", t->tree);
} catch (...) { return hprt::HandleException(); }
// The fork's "rbspkd" accelerator (RBSPKd): the RBSP tree's checks and layout, walked by the rbspkd walk with its kd counter pair
int hprt_scene_attach_rbspkd(HprtScene *s, const HprtRbspKd *t) try {
    if (!s || !t) return SetError(HPRT_E_INVALID, "hprt_scene_attach_rbspkd: null argument");
    return AttachRbsp(s, HprtScene::Walk::RbspKd, "rbspkd tree", t->tree);
} catch (...) { return hprt::HandleException(); }

// The fork's "bsppaper" accelerator (BSPPaper): GenericBSP's node array with M = 1 and a split axis per node, walked by the general
// BSP walk (device/bsppaper_walk.hip)
int hprt_scene_attach_bsppaper(HprtScene *s, const HprtBspPaper *t) try {
    if (!s || !t) return SetError(HPRT_E_INVALID, "hprt_scene_attach_bsppaper: null argument");
    const BspPaperTree &bt = t->tree;
    return AttachTree(s, HprtScene::Walk::BspPaper, {"bsppaper tree", bt.nodes, bt.primIndices, bt.nPrims, bt.bounds, BSPPAPER_M, nullptr,
                                                     (uint32_t)BSPPAPER_TODO_MAX, [&](uint32_t *depth) { return CheckBspPaperTree(bt, depth); }, &bt.axes});
} catch (...) { return hprt::HandleException(); }

// The fork's "bsppaperkd" accelerator (BSPPaperKd): the general BSP tree's layout with BSPKdNode's flags, walked by the kd-aware
// general BSP walk (device/bsppaperkd_walk.hip) with its kd counter pair
int hprt_scene_attach_bsppaperkd(HprtScene *s, const HprtBspPaperKd *t) try {
    if (!s || !t) return SetError(HPRT_E_INVALID, "hprt_scene_attach_bsppaperkd: null argument");
    const BspPaperTree &bt = t->tree;
    return AttachTree(s, HprtScene::Walk::BspPaperKd, {"bsppaperkd tree", bt.nodes, bt.primIndices, bt.nPrims, bt.bounds, 3u, nullptr,
                                                       (uint32_t)BSPPAPERKD_TODO_MAX, [&](uint32_t *depth) { return CheckBspPaperKdTree(bt, depth); }, &bt.axes,
                                                       BSPPAPERKD_OFF, BSPPAPERKD_LEAF});
} catch (...) { return hprt::HandleException(); }

// Two-level trees (pbrtObjectInstance, core/api.cpp:1794-1819): what AttachTwoLevel takes besides the handle's trees, which it
// reads as TreeView names a tree — through nodes, primIndices, nPrims and bounds
extern "C++" template <class Tree> struct TwoLevelView {
    const char *what;                                           // the tree's name in messages: "kd-tree", "RBSP tree"
    const HprtTwoLevel<Tree> &t;
    const char *(*check)(const Tree &, uint32_t *depth);        // CheckKdTree, CheckRbspTree
    uint32_t off, mask, leafTag;                                // the node layout: flag bits, their mask, a leaf's tag
    uint32_t todoMax;                                           // the entries the walk's one todo list holds
    std::function<std::string(const Tree &)> objectCheck;       // optional: what else is wrong with an object's tree ("": nothing)
    // optional: a tree's per-node split axes, 3 floats per node (bsppaper, bsppaperkd: BspPaperTree::axes).  When present the
    // attach uploads one float4 {x, y, z, 0} per node of the shared node array into HprtScene::treeAxes, in the array's order
    std::function<const std::vector<float> &(const Tree &)> axes;
};
// The top-level tree and every object's tree go through AttachTree's steps — the structural check, the todo-list rule (here over
// both levels), AppendTree, UploadTree, FillTree — into ONE node array and ONE primitiveIndices array with one DevInstEntry per
// instance (device/two_level.h); d: the walk's descriptor (DevKdInst, DevRbspInst), of which the shared fields are filled.  A
// view with axes concatenates them as it concatenates the nodes — the top-level tree's first, then each object's, and a zero entry
// of its own for the one-primitive leaf that stands for a tree-less object, so that the array has exactly as many entries as the
// node array and a 16-byte fetch beside ANY node's word, that leaf's included (it may be the array's last), stays inside it.  A
// refusal leaves the attached walk in place, a failed upload the BVH; on success the scene still walks its BVH and the caller,
// having filled the descriptor's own fields, sets its walk.
extern "C++" template <class Tree, class Dev> static int AttachTwoLevel(HprtScene *s, const TwoLevelView<Tree> &v, Dev &d) {
    const HprtTwoLevel<Tree> &t = v.t;
    const std::string what = v.what;
    const size_t nObjects = s->objectOrder.size();
    if (t.objects.size() != nObjects || t.instanceObject != s->instanceObject)
        return SetError(HPRT_E_INVALID, "the two-level " + what + " holds " + std::to_string(t.objects.size()) + " objects and " + std::to_string(t.instanceObject.size()) +
                                        " instances, the scene " + std::to_string(nObjects) + " and " + std::to_string(s->instanceObject.size()) + " (or they name other objects)");
    if (t.top.nPrims != s->topOrder.size())
        return SetError(HPRT_E_INVALID, "the top-level " + what + " holds " + std::to_string(t.top.nPrims) + " primitives, the scene " + std::to_string(s->topOrder.size()));
    if (v.axes && v.axes(t.top).size() != 3 * t.top.nodes.size()) return SetError(HPRT_E_INVALID, "the top-level " + what + " has not one split axis per node");
    uint32_t topDepth = 0, objectDepth = 0;
    uint64_t nNodes = t.top.nodes.size(), nIdx = t.top.primIndices.size();
    const char *bad = v.check(t.top, &topDepth);
    if (*bad) return SetError(HPRT_E_INVALID, "malformed top-level " + what + ": " + bad);
    for (size_t o = 0; o < nObjects; ++o) {
        const Tree &k = t.objects[o];
        if (k.nPrims != s->objectOrder[o].size())
            return SetError(HPRT_E_INVALID, "the " + what + " of object " + std::to_string(o) + " holds " + std::to_string(k.nPrims) + " primitives, the scene's object " + std::to_string(s->objectOrder[o].size()));
        if ((k.nPrims > 1) != !k.nodes.empty()) return SetError(HPRT_E_INVALID, "object " + std::to_string(o) + ": exactly the objects of more than one primitive have a tree");
        if (v.axes && v.axes(k).size() != 3 * k.nodes.size()) return SetError(HPRT_E_INVALID, "object " + std::to_string(o) + ": not one split axis per node");
        const std::string wrong = v.objectCheck ? v.objectCheck(k) : std::string();
        if (!wrong.empty()) return SetError(HPRT_E_INVALID, "object " + std::to_string(o) + ": " + wrong);
        nNodes += k.nodes.empty() ? 1u : k.nodes.size(); nIdx += k.primIndices.size();
        if (k.nodes.empty()) continue;
        uint32_t depth = 0;
        bad = v.check(k, &depth);
        if (*bad) return SetError(HPRT_E_INVALID, "malformed " + what + " of object " + std::to_string(o) + ": " + bad);
        objectDepth = std::max(objectDepth, depth);
    }
    if ((uint64_t)topDepth + objectDepth + 1u > v.todoMax)
        return SetError(HPRT_E_UNSUPPORTED, "two-level " + what + ": top-level depth " + std::to_string(topDepth) + " + deepest object depth " + std::to_string(objectDepth) +
                                            " + 1 is more than the walk's todo list holds (" + std::to_string(v.todoMax) + ")");
    if (nNodes > (0xffffffffull >> v.off) || nIdx > 0xffffffffull)
        return SetError(HPRT_E_UNSUPPORTED, "two-level " + what + ": more nodes over all trees than aboveChild can name");
    std::vector<uint2> nodes; std::vector<uint32_t> prims;
    nodes.reserve((size_t)nNodes); prims.reserve((size_t)nIdx);
    std::vector<float4> axes;
    if (v.axes) axes.reserve((size_t)nNodes);
    auto append = [&](const Tree &k, const std::vector<uint32_t> &order, uint32_t primBase) {
        if (v.axes) {
            const std::vector<float> &a = v.axes(k);
            for (size_t n = 0; n < k.nodes.size(); ++n) axes.push_back(make_float4(a[3 * n], a[3 * n + 1], a[3 * n + 2], 0.f));
        }
        return AppendTree(k.nodes, k.primIndices, InvertOrder(order, primBase), v.off, v.mask, v.leafTag, &nodes, &prims);
    };
    append(t.top, s->topOrder, 0u);
    std::vector<uint32_t> objectRoot(nObjects);
    for (size_t o = 0; o < nObjects; ++o) {
        const Tree &k = t.objects[o];
        if (!k.nodes.empty()) objectRoot[o] = append(k, s->objectOrder[o], s->objectPrimBase[o]);
        else {      // the lone primitive (or nothing: no instance names an empty object) as a one-primitive leaf
            objectRoot[o] = (uint32_t)nodes.size();
            nodes.push_back(make_uint2(s->objectPrimBase[o], v.leafTag | ((k.nPrims ? 1u : 0u) << v.off)));
            if (v.axes) axes.push_back(make_float4(0.f, 0.f, 0.f, 0.f));
        }
    }
    if (v.axes && axes.size() != nodes.size()) return SetError(HPRT_E_INVALID, "two-level " + what + ": " + std::to_string(axes.size()) + " split axes for " + std::to_string(nodes.size()) + " nodes");
    std::vector<DevInstEntry> entries(t.instanceObject.size());
    for (size_t i = 0; i < entries.size(); ++i) {
        const size_t o = (size_t)t.instanceObject[i];
        const Tree &k = t.objects[o];
        DevInstEntry &e = entries[i];
        for (int a = 0; a < 3; ++a) { e.lo[a] = k.bounds[a]; e.hi[a] = k.bounds[3 + a]; }
        e.root = objectRoot[o];
        e.prim = k.nodes.empty() ? (int32_t)s->objectPrimBase[o] : -1;
    }
    if (int rc = UploadTree(s, nodes, prims)) return rc;
    HIP_TRY(upload(s->instEntries, entries));
    if (v.axes) HIP_TRY(upload(s->treeAxes, axes));
    d = Dev{};
    FillTree(d, s, nodes.size(), prims.size(), t.top.bounds, topDepth + objectDepth + 1u);
    d.entries = s->instEntries.as<DevInstEntry>(); d.nEntries = (uint32_t)entries.size();
    return HPRT_OK;
}

// Two-level kd-trees (under Accelerator "kdtree"; device/kdinst_walk.h).  KdAccelNode: two flag bits, leaves tagged 3.
int hprt_scene_attach_kdinst(HprtScene *s, const HprtKdInst *t) try {
    if (!s || !t) return SetError(HPRT_E_INVALID, "hprt_scene_attach_kdinst: null argument");
    if (!s->instanced) return SetError(HPRT_E_UNSUPPORTED, "hprt_scene_attach_kdinst: the scene has no object instances; attach its kd-tree with hprt_scene_attach_kdtree");
    HIP_TRY(hipSetDevice(s->device));
    SceneCall call(s, nullptr);
    if (int rc = AttachTwoLevel(s, TwoLevelView<KdTree>{"kd-tree", *t, CheckKdTree, 2u, 3u, 3u, (uint32_t)KD_TODO_MAX, nullptr}, s->kdinst)) return rc;
    s->walk = HprtScene::Walk::KdInst;
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }

// Two-level RBSP trees (under Accelerator "rbsp" / "rbspkd"; device/rbspinst_walk.h): M directions — off flag bits, leaves tagged
// M — for every tree, the shared direction table and, for kd-aware trees, the rbspkd walk's kd counter pair.
int hprt_scene_attach_rbspinst(HprtScene *s, const HprtRbspInst *t) try {
    if (!s || !t) return SetError(HPRT_E_INVALID, "hprt_scene_attach_rbspinst: null argument");
    if (!s->instanced)
        return SetError(HPRT_E_UNSUPPORTED, "hprt_scene_attach_rbspinst: the scene has no object instances; attach its tree with hprt_scene_attach_rbsp / hprt_scene_attach_rbspkd");
    HIP_TRY(hipSetDevice(s->device));
    SceneCall call(s, nullptr);
    const uint32_t M = t->top.M, off = RbspBitOffset(M), mask = RbspBitMask(M);
    auto sameM = [M](const RbspTree &r) {
        return r.M == M ? std::string() : "its tree is over " + std::to_string(r.M) + " directions, the top-level tree over " + std::to_string(M);
    };
    DevRbspInst &d = s->rbspinst;
    if (int rc = AttachTwoLevel(s, TwoLevelView<RbspTree>{"RBSP tree", *t, CheckRbspTree, off, mask, M, (uint32_t)RBSP_TODO_MAX, sameM}, d)) return rc;
    if (t->kdAware)
        if (int rc = ResetKdShare(s)) return rc;
    d.M = M; d.off = off; d.mask = mask;
    for (uint32_t k = 0; k < 3 * M; ++k) d.dirs[k] = t->top.directions[k];
    d.kdCounters = t->kdAware ? s->kdShare.as<unsigned long long>() : nullptr;
    s->walk = t->kdAware ? HprtScene::Walk::RbspKdInst : HprtScene::Walk::RbspInst;
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }

// Two-level general BSP trees (under Accelerator "bsppaper" / "bsppaperkd"; device/bsppaperinst_walk.h): BSPNode's layout (one flag
// bit, leaves tagged 1) or, kd-aware, BSPKdNode's (three flag bits, leaves tagged 3) for every tree, one split axis per node of the
// shared array in treeAxes and, for kd-aware trees, the bsppaperkd walk's kd counter pair.
int hprt_scene_attach_bsppaperinst(HprtScene *s, const HprtBspPaperInst *t) try {
    if (!s || !t) return SetError(HPRT_E_INVALID, "hprt_scene_attach_bsppaperinst: null argument");
    if (!s->instanced)
        return SetError(HPRT_E_UNSUPPORTED, "hprt_scene_attach_bsppaperinst: the scene has no object instances; attach its tree with hprt_scene_attach_bsppaper / hprt_scene_attach_bsppaperkd");
    HIP_TRY(hipSetDevice(s->device));
    SceneCall call(s, nullptr);
    const bool kd = t->kdAware;
    auto sameLayout = [kd](const BspPaperTree &b) {
        return b.kdAware == kd ? std::string() : std::string(b.kdAware ? "its tree holds BSPKdNode's flags, the handle is not kd-aware" : "its tree holds BSPNode's flags, the handle is kd-aware");
    };
    if (t->top.kdAware != kd) return SetError(HPRT_E_INVALID, "the top-level tree's node layout is not the handle's");
    const TwoLevelView<BspPaperTree> view{kd ? "bsppaperkd tree" : "bsppaper tree", *t, kd ? CheckBspPaperKdTree : CheckBspPaperTree,
                                          kd ? (uint32_t)BSPPAPERKD_OFF : (uint32_t)BSPPAPER_OFF, kd ? (uint32_t)BSPPAPERKD_MASK : (uint32_t)BSPPAPER_MASK,
                                          kd ? (uint32_t)BSPPAPERKD_LEAF : 1u, kd ? (uint32_t)BSPPAPERKD_TODO_MAX : (uint32_t)BSPPAPER_TODO_MAX, sameLayout,
                                          [](const BspPaperTree &b) -> const std::vector<float> & { return b.axes; }};
    DevBspPaperInst &d = s->bsppaperinst;
    if (int rc = AttachTwoLevel(s, view, d)) return rc;
    if (kd)
        if (int rc = ResetKdShare(s)) return rc;
    d.axes = s->treeAxes.as<float4>();
    d.kdCounters = kd ? s->kdShare.as<unsigned long long>() : nullptr;
    s->walk = kd ? HprtScene::Walk::BspPaperKdInst : HprtScene::Walk::BspPaperInst;
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }

int hprt_scene_kd_counters(HprtScene *s, uint64_t out[2]) try {
    if (!s || !out) return SetError(HPRT_E_INVALID, "hprt_scene_kd_counters: null argument");
    HIP_TRY(hipSetDevice(s->device));
    SceneCall call(s, nullptr);
    out[0] = out[1] = 0;
    if (!CountsKdShare(s)) return HPRT_OK;
    unsigned long long c[2];
    HIP_TRY(hipMemcpy(c, s->kdShare.p, sizeof(c), hipMemcpyDeviceToHost));
    out[0] = c[0]; out[1] = c[1];
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }

void hprt_scene_destroy(HprtScene *s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    delete s;
}

// ---------------------------------------------------------------------------
// batched Aggregate calls
// ---------------------------------------------------------------------------
static void ReadCounters(HprtScene *s, bool anyHit, uint64_t out[4]) {
    DevCounters c;
    (void)hipMemcpy(&c, s->counters.p, sizeof(c), hipMemcpyDeviceToHost);
    if (!anyHit) { out[0] = c.nodesFetched; out[1] = c.nodesEntered; out[2] = c.triTests; out[3] = c.sphereTests; }
    else { out[0] = c.nodesFetchedP; out[1] = c.nodesEnteredP; out[2] = c.triTestsP; out[3] = c.sphereTestsP; }
}
// Stream copies for the plane-layout entry points ([7][n] rays in; t, prim, [3][n] barycentrics out)
static int ApiStreams(HprtScene *s, size_t n, RayStream *rays, HitStream *hits) {
    HIP_TRY(s->apiRays.alloc(32 * n + 256));
    HIP_TRY(s->apiHits.alloc(24 * n + 256));
    rays->a = s->apiRays.as<float4>(); rays->b = rays->a + n;
    hits->a = s->apiHits.as<float4>(); hits->b = (float2 *)(hits->a + n);
    return HPRT_OK;
}

int hprt_intersect_device(HprtScene *s, size_t n, const float *d_rays7, float *d_t, int32_t *d_prim, float *d_bary3, void *stream) try {
    if (!s || (n && (!d_rays7 || !d_t || !d_prim))) return SetError(HPRT_E_INVALID, "hprt_intersect_device: null argument");
    if (n > 0x7ffffff0ull) return SetError(HPRT_E_INVALID, "too many rays in one call");
    if (n == 0) return HPRT_OK;
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    SceneCall call(s, st);
    RayStream rays; HitStream hits;
    int rc = ApiStreams(s, n, &rays, &hits);
    if (rc != HPRT_OK) return rc;
    LaunchPackRays(st, d_rays7, (uint32_t)n, rays);
    Trace(s, st, false, false, nullptr, nullptr, (uint32_t)n, (uint32_t)n, rays, hits, nullptr, nullptr, s->workCounter.as<uint32_t>());
    LaunchUnpackHits(st, hits, (uint32_t)n, d_t, d_prim, d_bary3);
    call.leave_async();
    HIP_TRY(hipGetLastError());
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
int hprt_occluded_device(HprtScene *s, size_t n, const float *d_rays7, uint8_t *d_occ, void *stream) try {
    if (!s || (n && (!d_rays7 || !d_occ))) return SetError(HPRT_E_INVALID, "hprt_occluded_device: null argument");
    if (n > 0x7ffffff0ull) return SetError(HPRT_E_INVALID, "too many rays in one call");
    if (n == 0) return HPRT_OK;
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    SceneCall call(s, st);
    RayStream rays; HitStream hits;
    int rc = ApiStreams(s, n, &rays, &hits);
    if (rc != HPRT_OK) return rc;
    LaunchPackRays(st, d_rays7, (uint32_t)n, rays);
    HitStream none; none.a = nullptr; none.b = nullptr;
    Trace(s, st, true, false, nullptr, nullptr, (uint32_t)n, (uint32_t)n, rays, none, d_occ, nullptr, s->workCounter.as<uint32_t>());
    call.leave_async();
    HIP_TRY(hipGetLastError());
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }


static int TraceHost(HprtScene *s, bool anyHit, size_t n, const float *o, const float *d, const float *tmax, float *t_out,
                     int32_t *prim_out, int32_t *inst_out, float *bary_out, uint8_t *occ_out, uint64_t counters[4]) {
    if (!s || (n && (!o || !d || !tmax))) return SetError(HPRT_E_INVALID, "trace: null argument");
    if (n > 0x7ffffff0ull) return SetError(HPRT_E_INVALID, "too many rays in one call");
    if (n == 0) { if (counters) memset(counters, 0, 32); return HPRT_OK; }
    HIP_TRY(hipSetDevice(s->device));
    SceneCall call(s, nullptr);      // (blocking call on the null stream: ends in hipDeviceSynchronize)
    std::vector<float4> ra(n), rb(n);
    for (size_t i = 0; i < n; ++i) {
        ra[i] = make_float4(o[3 * i], o[3 * i + 1], o[3 * i + 2], tmax[i]);
        rb[i] = make_float4(d[3 * i], d[3 * i + 1], d[3 * i + 2], 0.f);
    }
    RayStream rays; HitStream hits;
    int rc = ApiStreams(s, n, &rays, &hits);
    if (rc != HPRT_OK) return rc;
    HIP_TRY(hipMemcpy(rays.a, ra.data(), 16 * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(rays.b, rb.data(), 16 * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(s->counters.p, 0, sizeof(DevCounters)));
    if (CountsKdShare(s)) HIP_TRY(hipMemset(s->kdShare.p, 0, 2 * sizeof(unsigned long long)));
    const bool count = counters != nullptr;
    if (!anyHit) {
        Trace(s, nullptr, false, count, nullptr, nullptr, (uint32_t)n, (uint32_t)n, rays, hits, nullptr, s->counters.as<DevCounters>(), s->workCounter.as<uint32_t>());
        HIP_TRY(hipGetLastError()); HIP_TRY(hipDeviceSynchronize());
        std::vector<float4> ha(n); std::vector<float2> hb(n);
        HIP_TRY(hipMemcpy(ha.data(), hits.a, 16 * n, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(hb.data(), hits.b, 8 * n, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) {
            if (t_out) t_out[i] = hit_t(hb[i]);
            if (prim_out) prim_out[i] = hit_prim(hit_word(ha[i]));
            if (inst_out) inst_out[i] = hit_inst(hb[i]);
            if (bary_out) { bary_out[3 * i] = hit_b0(ha[i]); bary_out[3 * i + 1] = hit_b1(ha[i]); bary_out[3 * i + 2] = hit_b2(ha[i]); }
        }
    } else {
        DevBuf outOcc;
        HIP_TRY(outOcc.alloc(n));
        HitStream none; none.a = nullptr; none.b = nullptr;
        Trace(s, nullptr, true, count, nullptr, nullptr, (uint32_t)n, (uint32_t)n, rays, none, outOcc.as<uint8_t>(), s->counters.as<DevCounters>(), s->workCounter.as<uint32_t>());
        HIP_TRY(hipGetLastError()); HIP_TRY(hipDeviceSynchronize());
        if (occ_out) HIP_TRY(hipMemcpy(occ_out, outOcc.p, n, hipMemcpyDeviceToHost));
    }
    if (counters) ReadCounters(s, anyHit, counters);
    return HPRT_OK;
}
int hprt_intersect(HprtScene *s, size_t n, const float *o, const float *d, const float *tmax, float *t_out, int32_t *prim_out,
                   float *bary_out, uint64_t counters[4]) try {
    return TraceHost(s, false, n, o, d, tmax, t_out, prim_out, nullptr, bary_out, nullptr, counters);
} catch (...) { return hprt::HandleException(); }
int hprt_intersect_instanced(HprtScene *s, size_t n, const float *o, const float *d, const float *tmax, float *t_out, int32_t *prim_out,
                             int32_t *inst_out, float *bary_out, uint64_t counters[4]) try {
    return TraceHost(s, false, n, o, d, tmax, t_out, prim_out, inst_out, bary_out, nullptr, counters);
} catch (...) { return hprt::HandleException(); }
int hprt_occluded(HprtScene *s, size_t n, const float *o, const float *d, const float *tmax, uint8_t *occ, uint64_t counters[4]) try {
    return TraceHost(s, true, n, o, d, tmax, nullptr, nullptr, nullptr, nullptr, occ, counters);
} catch (...) { return hprt::HandleException(); }

// ---------------------------------------------------------------------------
// Render
// ---------------------------------------------------------------------------
namespace {

// words of s->queueCounts (EnsureWorkspace): the two QueueSets' counters [0, 512), the bins' [512, 1024), then k_repair's two test counters
constexpr size_t kSpecCountsAt = 1024;
struct BatchTimers { double extendMs = 0, occludedMs = 0; uint64_t extendLaunches = 0, occludedLaunches = 0, extendRays = 0, occludedRays = 0; };

// Runs the bounce loop for one batch of nSlots freshly generated paths.
// pixelStats (or null): [6][nPix] per-pixel counters of the local pixels, fed from the per-ray counts of every trace
//
// Per bounce b:   trace(path b) -> bin -> shade x3 -> [counts to the host] -> trace(shadow b) | trace(MIS b) | trace(path b+1)
//                 -> resolve(b) (vertices with an MIS ray, if any) -> repair(b) -> bin(b+1) ...
// repair(b) sets right the speculated vertices of b whose shadow ray was blocked AND whose path ends there (QueueSet::end; no launch when
// there are none).  A blocked speculated vertex whose path goes on is set right where its radiance is read next: bin(b+1) for a path that
// ends at the bin, else shade(b+1) — they take the record of plane b & 1 instead of out.L when the segment carries RAY_FOLD_MARK and
// occluded[] is set, while shade(b+1) writes its own records to the other plane.  HPRT_FOLD_REPAIR=0, or a render that counts the
// speculated vertices, sends every shadow ray of b through repair(b) as before and marks nothing.
// The three traces that follow a shading pass depend on nothing but that pass.  Running them on three HIP streams (so that
// each fills the tails of the others' persistent kernels) was built and measured in round 2: SLOWER — atrium 1024 spp
// 1064 -> 1119 ms, living room 455 -> 478 ms, killeroo-simple 90.6 -> 91.8 ms (every persistent kernel is sized to fill the
// machine, so the second and third only get wave slots as the first one's blocks drain, and the cross-stream waits add
// bubbles) — and removed again: every kernel runs on the caller's stream, where HIP-event times are exclusive.
int RunBatch(HprtScene *s, hipStream_t st, const RenderParams &rpIn, const Workspace &w, const QueueSet &qa, const QueueSet &qb,
             const BinSet &bins, uint32_t s0, uint32_t nSlots, bool count, EventTimer &ev, BatchTimers *bt, HprtRenderStats *stats,
             uint32_t *pixelStats = nullptr, const IrregularSink *irregular = nullptr) {
    uint4 *rayStats = pixelStats ? s->rayStats.as<uint4>() : nullptr;
    // Speculated light samples (k_shade, k_repair).  Per-pixel-statistics renders keep the full path: they read pendBeta.w of every shadow
    // ray as a plain path id.  So does a batch whose path ids would reach the record's flag bits.
    RenderParams rp = rpIn;
    rp.speculate = SpeculateLightEnabled() && !pixelStats && !rayStats && nSlots <= SPEC_MAX_PATHS ? 1 : 0;
    assert(!rp.speculate || nSlots <= SPEC_MAX_PATHS);
    // Folded repair: a blocked speculated vertex whose path goes on is set right by the next bounce's reader of its radiance (k_shade, k_bin:
    // RAY_FOLD_MARK), and k_repair runs over the vertices at which a path ends (QueueSet::end) alone.  A counting render of the tests
    // (shadeCountsOn) keeps every shadow ray in k_repair: that is where the speculated and the repaired vertices are counted.
    rp.foldRepair = rp.speculate && FoldRepairEnabled() && !s->shadeCountsOn ? 1 : 0;
    uint32_t *specCounts = rp.speculate && s->shadeCountsOn ? s->queueCounts.as<uint32_t>() + kSpecCountsAt : nullptr;
    if (specCounts) HIP_TRY(hipMemsetAsync(specCounts, 0, 2 * sizeof(uint32_t), st));
    uint32_t *pixelKd = pixelStats && CountsKdShare(s) ? s->pixelKdLocal.as<uint32_t>() : nullptr;     // the rbspkd / bsppaperkd walk's kd share
    uint32_t *wcPath = s->workCounter.as<uint32_t>();
    LaunchGenerate(st, s->dev, rp, w.path[0], s0, nSlots, irregular);
    const uint32_t *activeQ = nullptr; uint32_t active = nSlots;
    QueueSet q[2] = {qa, qb};
    DevCounters *ctr = s->counters.as<DevCounters>();
    std::vector<std::pair<hipEvent_t, hipEvent_t>> evExt, evOcc;
    auto tracePath = [&](int bounce) -> int {      // closest hits of the path segments entering bounce `bounce`
        const PathStream &in = w.path[bounce & 1];
        hipEvent_t e0 = ev.get(), e1 = ev.get();
        HIP_TRY(hipEventRecord(e0, st));
        Trace(s, st, false, count, activeQ, nullptr, active, active, in.ray, w.hit, nullptr, ctr, wcPath, rayStats);
        if (pixelStats) LaunchPixelStats(st, rayStats, bounce == 0 ? nullptr : in.beta, activeQ, nullptr, active, active, rp.nPix, false, pixelStats);
        if (pixelKd) LaunchPixelKdStats(st, rayStats, bounce == 0 ? nullptr : in.beta, activeQ, nullptr, active, active, rp.nPix, false, pixelKd);
        HIP_TRY(hipEventRecord(e1, st));
        evExt.push_back({e0, e1}); bt->extendRays += active; ++bt->extendLaunches;
        stats->rays += active;
        return HPRT_OK;
    };
    if (active > 0) { int rc = tracePath(0); if (rc != HPRT_OK) return rc; }
    for (int bounce = 0; active > 0; ++bounce) {
        const QueueSet &cur = q[bounce & 1];
        const PathStream &in = w.path[bounce & 1], &out = w.path[(bounce + 1) & 1];
        // this bounce's records go to one plane while its readers (k_bin, k_shade) still find the bounce before's in the other
        VertexStreams vs = w.vs;
        vs.pendBeta = w.pend[bounce & 1]; vs.pendPrev = w.pend[(bounce + 1) & 1];
        HIP_TRY(hipMemsetAsync(cur.nextCount, 0, 256 * sizeof(uint32_t), st));   // the five counters (EnsureWorkspace)
        HIP_TRY(hipMemsetAsync(bins.count, 0, 8 * BIN_STRIDE * sizeof(uint32_t), st));
        LaunchBin(st, s->dev, in, w.hit, activeQ, nullptr, active, active, rp.maxDepth, bounce, bins, w.Lfinal, vs, rp.foldRepair != 0);
        HIP_TRY(hipMemcpyAsync(bins.count + 5 * BIN_STRIDE, bins.count + 2 * BIN_STRIDE, sizeof(uint32_t), hipMemcpyDeviceToDevice, st));   // bin 2 before deferrals
        // one launch per material bin; grids are sized for the upper bound, surplus blocks exit on the bin's count
        // (the specialised variants first: they may hand vertices over to the generic one; bin 3: vertices on image-textured materials)
        static const int order[5] = {BIN_MATTE, BIN_PLASTIC, BIN_SUBSTRATE, BIN_GENERIC, BIN_TEXTURED};
        for (int k = 0; k < (s->dev.textures ? 5 : 4); ++k) {
            const int mode = order[k];
            if (mode == (int)BIN_SUBSTRATE && !s->hasSubstrateBin) continue;
            LaunchShade(st, mode, s->dev, rp, in, w.hit, active, s0, out, vs, cur, bins, w.Lfinal, bounce == 0);
        }
        HIP_TRY(hipMemcpyAsync(s->hostCounts + 4096, cur.nextCount, 256 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        if (s->shadeCountsOn) {      // (tests only) bin 2 after the deferrals and as binned
            HIP_TRY(hipMemcpyAsync(s->hostCounts + 12, bins.count + 2 * BIN_STRIDE, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(s->hostCounts + 13, bins.count + 5 * BIN_STRIDE, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        }
        if (s->dev.voxSlot) {      // on-demand SpatialLightDistribution: vertices whose voxel had no distribution yet wait in the retry lists
            HIP_TRY(hipMemcpyAsync(s->hostCounts + 16, bins.count + 6 * BIN_STRIDE, 2 * BIN_STRIDE * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(s->hostCounts + 15, s->dev.voxRequestCount, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            const uint32_t nRetry[2] = {s->hostCounts[16], s->hostCounts[16 + BIN_STRIDE]}, nReq = s->hostCounts[15];
            if (s->shadeCountsOn) s->shadeRetried += (uint64_t)nRetry[0] + nRetry[1];
            if (nRetry[0] + nRetry[1] > 0) {
                if ((uint64_t)s->voxRowsUsed + nReq > s->voxRows)
                    return SetError(HPRT_E_UNSUPPORTED, "spatial light distribution: the paths touch more voxels than the row pool holds (" + std::to_string(s->voxRows) +
                                                        " rows of " + std::to_string(s->dev.nLights) + " lights; HPRT_VOXEL_POOL_MB raises it, or use \"power\" / \"uniform\")");
                // SpatialLightDistribution::ComputeDistribution for the voxels just asked for, then the waiting vertices again
                LaunchVoxelFill(st, s->dev, s->voxRi.as<float>(), nReq, s->voxRowsUsed, s->voxFunc.as<float>(), s->voxCdf.as<float>(), s->voxFuncInt.as<float>());
                s->voxRowsUsed += nReq;
                HIP_TRY(hipMemsetAsync(s->dev.voxRequestCount, 0, sizeof(uint32_t), st));
                for (int r = 0; r < 2; ++r)
                    if (nRetry[r]) LaunchShade(st, 2 + r, s->dev, rp, in, w.hit, nRetry[r], s0, out, vs, cur, bins, w.Lfinal, bounce == 0, true);
                HIP_TRY(hipMemcpyAsync(s->hostCounts + 4096, cur.nextCount, 256 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            }
        }
        HIP_TRY(hipStreamSynchronize(st));
        if (s->shadeCountsOn) s->shadeDeferred += s->hostCounts[12] - s->hostCounts[13];
        const uint32_t nNext = s->hostCounts[4096], nShadow = s->hostCounts[4096 + 64], nMis = s->hostCounts[4096 + 128], nResolve = s->hostCounts[4096 + 192];
        const uint32_t nEnd = s->hostCounts[4096 + 32];
        if (s->capture.out7 && s->capture.bounce == bounce && s0 == 0) {      // diagnostics (hprt_debug_capture_rays)
            const uint32_t *cq = s->capture.kind == 0 ? cur.next : s->capture.kind == 1 ? cur.shadow : cur.mis;
            const uint32_t cn = s->capture.kind == 0 ? nNext : s->capture.kind == 1 ? nShadow : nMis;
            const RayStream &cs = s->capture.kind == 0 ? out.ray : s->capture.kind == 1 ? vs.shadow : vs.mis;
            LaunchCaptureRays(st, cq, cn, cs, s->capture.out7, (uint32_t)s->capture.cap);
            s->capture.n = std::min<size_t>(cn, s->capture.cap);
        }
        if (nShadow) {
            hipEvent_t a = ev.get(), b = ev.get();
            HIP_TRY(hipEventRecord(a, st));
            HitStream none; none.a = nullptr; none.b = nullptr;
            // a plain render of an eligible scene answers its shadow rays from its light's grid; counting, per-pixel-statistics and
            // trace-all renders keep the walk (their counters are the reference's node counts)
            if (GridInUse(s) && !count && !rayStats && rp.cullMis) {
                LaunchGrid(s, st, cur.shadow, nShadow, vs.shadow, vs.occluded, wcPath);
                ++s->gridInfo.renderLaunches;
            }
            else Trace(s, st, true, count, cur.shadow, nullptr, nShadow, nShadow, vs.shadow, none, vs.occluded, ctr, wcPath, rayStats);
            if (pixelStats) LaunchPixelStats(st, rayStats, vs.pendBeta, cur.shadow, nullptr, nShadow, nShadow, rp.nPix, true, pixelStats);
            if (pixelKd) LaunchPixelKdStats(st, rayStats, vs.pendBeta, cur.shadow, nullptr, nShadow, nShadow, rp.nPix, true, pixelKd);
            HIP_TRY(hipEventRecord(b, st));
            evOcc.push_back({a, b}); bt->occludedRays += nShadow; ++bt->occludedLaunches;
            stats->shadow_rays += nShadow;
        }
        if (nMis) {
            hipEvent_t a = ev.get(), b = ev.get();
            HIP_TRY(hipEventRecord(a, st));
            Trace(s, st, false, count, cur.mis, nullptr, nMis, nMis, vs.mis, vs.misHit, nullptr, ctr, wcPath, rayStats);
            if (pixelStats) LaunchPixelStats(st, rayStats, vs.pendBeta, cur.mis, nullptr, nMis, nMis, rp.nPix, false, pixelStats);
            if (pixelKd) LaunchPixelKdStats(st, rayStats, vs.pendBeta, cur.mis, nullptr, nMis, nMis, rp.nPix, false, pixelKd);
            HIP_TRY(hipEventRecord(b, st));
            evExt.push_back({a, b}); bt->extendRays += nMis; ++bt->extendLaunches;
            stats->rays += nMis;
        }
        activeQ = cur.next; active = nNext;
        // (maxDepth is bounded by CheckDepth, and no path outlives bounce maxDepth)
        if (active > 0 && bounce > rp.maxDepth) return SetError(HPRT_E_DEVICE, "internal error: paths are still active beyond maxdepth");
        // the full vertices' direct lighting, then the speculated vertices whose shadow ray was blocked (disjoint sets of vertices)
        if (nResolve) LaunchResolve(st, s->dev, vs, out.L, w.Lfinal, cur.resolve, cur.resolveCount, nResolve);
        if (rp.foldRepair) { if (nEnd) LaunchRepair(st, vs, out.L, w.Lfinal, cur.end, nEnd, nullptr); }
        else if (rp.speculate && nShadow) LaunchRepair(st, vs, out.L, w.Lfinal, cur.shadow, nShadow, specCounts);
        if (s->shadeCountsOn) s->shadeFull += nResolve;
        if (active > 0) { int rc = tracePath(bounce + 1); if (rc != HPRT_OK) return rc; }
    }
    HIP_TRY(hipGetLastError());
    if (specCounts) HIP_TRY(hipMemcpyAsync(s->hostCounts + 256, specCounts, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (specCounts) { s->shadeSpeculated += s->hostCounts[256]; s->shadeRepaired += s->hostCounts[257]; }
    for (auto &p : evExt) { float ms = 0; if (hipEventElapsedTime(&ms, p.first, p.second) == hipSuccess) bt->extendMs += ms; }
    for (auto &p : evOcc) { float ms = 0; if (hipEventElapsedTime(&ms, p.first, p.second) == hipSuccess) bt->occludedMs += ms; }
    ev.reset();
    return HPRT_OK;
}

// words of s->queues per path: two QueueSets of five index queues, the deferral indices (BinSet::aux) and five bins of 8-byte entries
constexpr size_t kQueueWordsPerSlot = 10 + 1 + 2 * N_BINS;
int EnsureWorkspace(HprtScene *s, size_t nSlots, Workspace *ps, QueueSet *qa, QueueSet *qb, BinSet *bins) {
    const bool instances = s->dev.nInstances != 0u;
    HIP_TRY(s->planes.alloc(PlaneBytes(nSlots, instances)));
    CarvePlanes(s->planes.as<char>(), nSlots, instances, ps);
    HIP_TRY(s->queues.alloc(kQueueWordsPerSlot * nSlots * sizeof(uint32_t) + 4096));
    HIP_TRY(s->queueCounts.alloc(2048 * sizeof(uint32_t)));
    uint32_t *qbase = s->queues.as<uint32_t>(), *cbase = s->queueCounts.as<uint32_t>();
    QueueSet *qs[2] = {qa, qb};
    for (int k = 0; k < 2; ++k) {
        qs[k]->next = qbase + (5 * k + 0) * nSlots; qs[k]->shadow = qbase + (5 * k + 1) * nSlots;
        qs[k]->mis = qbase + (5 * k + 2) * nSlots; qs[k]->resolve = qbase + (5 * k + 3) * nSlots; qs[k]->end = qbase + (5 * k + 4) * nSlots;
        // one counter per 256-byte line: atomics of different queues do not serialise on a shared line (the end queue's, rarely
        // touched, sits half a line behind nextCount: the set's 256 words are still cleared and copied to the host as one block)
        qs[k]->nextCount = cbase + 256 * k; qs[k]->shadowCount = cbase + 256 * k + 64; qs[k]->misCount = cbase + 256 * k + 128; qs[k]->resolveCount = cbase + 256 * k + 192;
        qs[k]->endCount = cbase + 256 * k + 32;
    }
    bins->aux = qbase + 10 * nSlots;
    for (int k = 0; k < (int)N_BINS; ++k) bins->q[k] = reinterpret_cast<uint2 *>(qbase + (11 + 2 * k) * nSlots + (nSlots & 1u));      // (8-byte entries, 8-byte aligned)
    bins->count = cbase + 512;
    bins->retry[0] = bins->retry[1] = nullptr;
    if (s->dev.voxSlot) {      // (on-demand voxel tables only)
        HIP_TRY(s->retryQueues.alloc(2 * nSlots * sizeof(uint2) + 256));
        bins->retry[0] = s->retryQueues.as<uint2>(); bins->retry[1] = bins->retry[0] + nSlots;
    }
    return HPRT_OK;
}

// Test hook: garbage in everything a render treats as scratch.  A render whose film changes under it has consumed a word
// it never wrote (a fresh allocation on a busy card holds other processes' data, not zeros).
int PoisonWorkspace(HprtScene *s) {
    if (s->poisonByte < 0) return HPRT_OK;
    hprt::DevBuf *bufs[] = {&s->planes, &s->queues, &s->Lall, &s->deepStack, &s->rayStats, &s->irregular, &s->aoSlots, &s->aoRays, &s->dlSlots, &s->dlRays};
    for (hprt::DevBuf *b : bufs) if (b->p && b->bytes) HIP_TRY(hipMemset(b->p, s->poisonByte, b->bytes));
    HIP_TRY(hipDeviceSynchronize());
    return HPRT_OK;
}

// Samples per pixel of one wavefront batch (see the comment at its use in hprt_render)
int ChooseBatch(HprtScene *s, int32_t sppChunk, uint32_t nPix, uint32_t spp, uint32_t *out) {
    uint32_t chunk;
    if (sppChunk > 0) chunk = (uint32_t)sppChunk;
    else {
        size_t freeB = 0, totalB = 0;
        HIP_TRY(hipMemGetInfo(&freeB, &totalB));
        freeB += s->planes.bytes + s->queues.bytes;                 // this scene's previous workspace is reused or released
        const size_t perPath = PlaneBytesPerSlot(s->dev.nInstances != 0u) + kQueueWordsPerSlot * sizeof(uint32_t);
        static const size_t capM = [] { const char *e = getenv("HPRT_BATCH_MPATHS"); return e ? (size_t)atoi(e) : (size_t)256; }();
        const size_t budget = std::min<size_t>(capM << 20, std::max<size_t>(freeB / 2 / perPath, 1ull << 20));
        chunk = std::max<uint32_t>(1u, (uint32_t)(budget / std::max<uint32_t>(nPix, 1u)));
        if ((uint64_t)chunk * nPix > 0x7fffffffull) chunk = (uint32_t)(0x7fffffffull / nPix);
        chunk = std::max(1u, std::min(chunk, spp));
        const uint32_t nBatches = (spp + chunk - 1) / chunk;
        chunk = (spp + nBatches - 1) / nBatches;                    // equal batches
    }
    chunk = std::min(chunk, spp);
    if ((uint64_t)chunk * nPix > 0x7fffffffull) chunk = (uint32_t)(0x7fffffffull / nPix);
    *out = chunk;
    return HPRT_OK;
}

// Host-side grouping of the irregular samples into per-destination lists, in the exact
// order the reference's tile loop would have added them (core/integrator.cpp:267-333).
struct ExtraEntry { uint32_t dest; uint32_t srcTile; uint32_t srcPos; uint32_t sample; uint32_t srcPix; uint8_t pre; };

// ---- Integrator "ambientocclusion" (device/ao.h): AOIntegrator::Li, integrators/ao.cpp:57-103 ----
// Hemisphere rays per any-hit launch: the buffer of fixed size a batch's rays go through, hit range by hit range (1.2 GB of rays,
// terms and bytes).  hprt_debug_ao_ray_capacity (tests) lowers it so that small renders take several ranges too.
constexpr size_t kAoRayCapacity = (size_t)1 << 25, kAoRayBytes = 32 + 4 + 1;
size_t g_aoRayCapacity = kAoRayCapacity;
// Camera samples per batch: 136 bytes each (ray, hit, hit record), 16 M of them unless the caller's spp_chunk says otherwise
constexpr size_t kAoSlotCapacity = (size_t)1 << 24;
struct AoWorkspace { RayStream cam; HitStream hit; AoRecords recs; uint32_t *hitCount; RayStream rays; float *term; uint8_t *occ; size_t rayCap; };
int CheckAoParams(const HprtAoParams *ao, int32_t spp, const char *fn) {
    if (!ao) return SetError(HPRT_E_INVALID, std::string(fn) + ": null argument");
    if (ao->n_samples < 1 || ao->n_samples > (int32_t)AO_MAX_SAMPLES)
        return SetError(HPRT_E_INVALID, std::string(fn) + ": n_samples must lie in 1..1024");
    if (spp <= 0) return SetError(HPRT_E_INVALID, "spp must be positive");
    if ((int64_t)ao->n_samples * (int64_t)spp > 0x7fffffffll)
        return SetError(HPRT_E_UNSUPPORTED, std::string(fn) + ": n_samples * spp exceeds INT32_MAX (the reference's int nSamples = size * samplesPerPixel "
                                            "overflows there, core/sampler.cpp:157)");
    return HPRT_OK;
}
int EnsureAoWorkspace(HprtScene *s, size_t nSlots, uint32_t nSamples, uint64_t maxRays, AoWorkspace *w) {
    const bool instances = s->dev.nInstances != 0u;
    HIP_TRY(s->aoSlots.alloc(nSlots * (32 + 16 + (instances ? 8 : 0) + 16 * AO_RECORD_PLANES) + 16 * 256));
    PlaneAllocator a{s->aoSlots.as<char>(), 0, 0};
    w->cam.a = a.take<float4>(nSlots); w->cam.b = a.take<float4>(nSlots);
    w->hit.a = a.take<float4>(nSlots); w->hit.b = instances ? a.take<float2>(nSlots) : nullptr;
    w->recs.rec = a.take<float4>(nSlots * AO_RECORD_PLANES); w->recs.stride = (uint32_t)nSlots;
    w->hitCount = a.take<uint32_t>(64);
    // never less than one hit's rays, never more than the render can produce
    w->rayCap = (size_t)std::min<uint64_t>(std::max<uint64_t>(g_aoRayCapacity, nSamples), std::max<uint64_t>(maxRays, nSamples));
    HIP_TRY(s->aoRays.alloc(w->rayCap * kAoRayBytes + 16 * 256));
    PlaneAllocator b{s->aoRays.as<char>(), 0, 0};
    w->rays.a = b.take<float4>(w->rayCap); w->rays.b = b.take<float4>(w->rayCap);
    w->term = b.take<float>(w->rayCap); w->occ = b.take<uint8_t>(w->rayCap);
    return HPRT_OK;
}
// One batch of nSlots camera samples: k_generate -> closest-hit trace -> k_ao_frame -> [hit count to the host] -> per range of hits
// whose rays fit the ray buffer: k_ao_rays -> any-hit trace -> k_ao_resolve.  The any-hit trace is the scene's walk whatever the
// scene: GridInUse is a property of the path render's light-directed rays, and these end at no light.
int RunAoBatch(HprtScene *s, hipStream_t st, const RenderParams &rp, const HprtAoParams &ao, const AoWorkspace &w, const uint64_t *aoBase, uint32_t s0,
               uint32_t nSlots, bool count, const AoRadiance &out, EventTimer &ev, BatchTimers *bt, HprtRenderStats *stats, const IrregularSink *irregular) {
    const uint32_t n = (uint32_t)ao.n_samples;
    PathStream camPath; camPath.ray = w.cam; camPath.beta = nullptr; camPath.L = nullptr;      // (k_generate stores the ray alone)
    DevCounters *ctr = s->counters.as<DevCounters>();
    uint32_t *wc = s->workCounter.as<uint32_t>();
    std::vector<std::pair<hipEvent_t, hipEvent_t>> evExt, evOcc, evAo[3];      // (evAo: the three kernels of device/ao.hip, for tools/bench_ao.py)
    auto timed = [&](std::vector<std::pair<hipEvent_t, hipEvent_t>> &into, auto launch) -> int {
        hipEvent_t e0 = ev.get(), e1 = ev.get();
        HIP_TRY(hipEventRecord(e0, st));
        launch();
        HIP_TRY(hipEventRecord(e1, st));
        into.push_back({e0, e1});
        return HPRT_OK;
    };
    LaunchGenerate(st, s->dev, rp, camPath, s0, nSlots, irregular);
    {
        hipEvent_t e0 = ev.get(), e1 = ev.get();
        HIP_TRY(hipEventRecord(e0, st));
        Trace(s, st, false, count, nullptr, nullptr, nSlots, nSlots, w.cam, w.hit, nullptr, ctr, wc);
        HIP_TRY(hipEventRecord(e1, st));
        evExt.push_back({e0, e1}); bt->extendRays += nSlots; ++bt->extendLaunches;
        stats->rays += nSlots;
    }
    HIP_TRY(hipMemsetAsync(w.hitCount, 0, sizeof(uint32_t), st));
    if (int rc = timed(evAo[0], [&] { LaunchAoFrame(st, s->dev, rp, w.cam, w.hit, nSlots, s0, n, aoBase, w.recs, w.hitCount, out); })) return rc;
    HIP_TRY(hipMemcpyAsync(s->hostCounts + 9, w.hitCount, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const uint32_t nHits = s->hostCounts[9];
    if (nHits > nSlots) return SetError(HPRT_E_DEVICE, "internal error: more ambient-occlusion hits than camera samples");
    const uint32_t hitsPerRange = (uint32_t)(w.rayCap / n);
    HitStream none; none.a = nullptr; none.b = nullptr;
    for (uint32_t h0 = 0; h0 < nHits; h0 += hitsPerRange) {
        const uint32_t nh = std::min(hitsPerRange, nHits - h0), nr = nh * n;
        if (int rc = timed(evAo[1], [&] { LaunchAoRays(st, s->dev, rp.hal, w.recs, h0, nh, n, ao.cos_sample != 0, w.rays, w.term); })) return rc;
        hipEvent_t a = ev.get(), b = ev.get();
        HIP_TRY(hipEventRecord(a, st));
        Trace(s, st, true, count, nullptr, nullptr, nr, nr, w.rays, none, w.occ, ctr, wc);
        HIP_TRY(hipEventRecord(b, st));
        evOcc.push_back({a, b}); bt->occludedRays += nr; ++bt->occludedLaunches;
        stats->shadow_rays += nr;
        if (int rc = timed(evAo[2], [&] { LaunchAoResolve(st, w.recs, h0, nh, n, w.occ, w.term, out); })) return rc;
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    for (auto &p : evExt) { float ms = 0; if (hipEventElapsedTime(&ms, p.first, p.second) == hipSuccess) bt->extendMs += ms; }
    for (auto &p : evOcc) { float ms = 0; if (hipEventElapsedTime(&ms, p.first, p.second) == hipSuccess) bt->occludedMs += ms; }
    for (int k = 0; k < 3; ++k)
        for (auto &p : evAo[k]) { float ms = 0; if (hipEventElapsedTime(&ms, p.first, p.second) == hipSuccess) s->aoKernelMs[k] += ms; }
    ev.reset();
    return HPRT_OK;
}

// ---- Integrator "directlighting" (device/direct.h): DirectLightingIntegrator::Li, integrators/directlighting.cpp:62-100 ----
// Light samples per pair of trace launches: the buffer of fixed size a step's light work goes through, hit range by hit range (121 bytes
// per item: its record, a shadow ray and its byte, a BSDF-sampled ray and its hit).  hprt_debug_dl_ray_capacity (tests) lowers it so
// that small renders take several ranges too.
constexpr size_t kDlRayCapacity = (size_t)1 << 24;
size_t g_dlRayCapacity = kDlRayCapacity;
// Camera samples per batch: 128 bytes per depth of stack and some 130 more each, 4 M of them unless the caller's spp_chunk says otherwise
constexpr size_t kDlSlotCapacity = (size_t)1 << 22;
// One hprt_render_direct / hprt_sample_direct call: the parameters as given, and the per-light counts (all 1 where the caller passed none)
struct DlJob { HprtDirectParams params; std::vector<int32_t> nLightSamples; };
struct DlWorkspace {
    DlParams dp; DlState state; DlRecords recs; DlItems items; DlRays rays;
    RayStream node[2]; uint32_t *live[2]; HitStream hit;
    uint32_t *counts;      // hit, shadow-ray, BSDF-ray and next-node counters, 64 words apart
    size_t itemCap;
};
// The worst case of the sampler's dimension cursor: the arrays, then every node of a full binary tree of maxDepth levels draws its plain
// light sample values (only the nodes behind the first maxDepth can find the arrays used up) and, above the last level, two Get2D
int64_t DirectWorstDimensions(int strategy, int64_t maxDepth, int64_t nLights) {
    const int64_t nodes = ((int64_t)1 << maxDepth) - 1, inner = ((int64_t)1 << (maxDepth - 1)) - 1;
    const int64_t lightDims = nLights == 0 ? 0 : strategy == 1 ? 5 * nodes : 4 * nLights * std::max<int64_t>(0, nodes - maxDepth);
    return 5 + (strategy == 0 ? 4 * maxDepth * nLights : 0) + lightDims + 4 * inner;
}
// Everything hprt_render_direct and hprt_sample_direct refuse, judged without touching the device
int CheckDirect(const HprtScene *s, const HprtDirectParams *p, const int32_t *nLightSamples, size_t nLights, int32_t spp, int32_t flags, const char *fn, DlJob *job) {
    const std::string f(fn);
    if (!p) return SetError(HPRT_E_INVALID, f + ": null argument");
    if (p->strategy != 0 && p->strategy != 1) return SetError(HPRT_E_INVALID, f + ": strategy must be 0 (all) or 1 (one)");
    if (p->max_depth < 1) return SetError(HPRT_E_INVALID, f + ": max_depth must be at least 1");
    if (spp <= 0) return SetError(HPRT_E_INVALID, "spp must be positive");
    if (nLightSamples) for (size_t j = 0; j < nLights; ++j) if (nLightSamples[j] < 1) return SetError(HPRT_E_INVALID, f + ": every light's sample count must be at least 1");
    if (p->max_depth > HPRT_DIRECT_MAX_DEPTH) return SetError(HPRT_E_UNSUPPORTED, f + ": max_depth above " + std::to_string(HPRT_DIRECT_MAX_DEPTH));
    if (flags & ~HPRT_RENDER_COUNT_WORK)
        return SetError(HPRT_E_UNSUPPORTED, f + ": only HPRT_RENDER_COUNT_WORK is supported (per-pixel statistics, EXPORT_FOREIGN, TRACE_ALL and COUNT_TRACED stay with hprt_render)");
    if (DirectWorstDimensions(p->strategy, p->max_depth, (int64_t)nLights) > 1000)
        return SetError(HPRT_E_UNSUPPORTED, f + ": with max_depth " + std::to_string(p->max_depth) + " and " + std::to_string(nLights) + " lights a camera sample's tree could pass "
                                            "the 1,000 sampler dimensions of the reference's Halton tables");
    uint64_t items = 0;
    for (size_t j = 0; j < nLights; ++j) {
        const int64_t n = nLightSamples ? nLightSamples[j] : 1;
        if (p->strategy == 0 && n * (int64_t)spp > 0x7fffffffll)
            return SetError(HPRT_E_UNSUPPORTED, f + ": a light's sample count * spp exceeds INT32_MAX (the reference's int nSamples = size * samplesPerPixel overflows "
                                                "there, core/sampler.cpp:157)");
        items += (uint64_t)n;
    }
    if (p->strategy == 0 && items > DL_MAX_ITEMS) return SetError(HPRT_E_UNSUPPORTED, f + ": more than 65,536 light samples per node");
    if (!s) return SetError(HPRT_E_INVALID, f + ": null argument");
    if (nLights != (size_t)s->dev.nLights)
        return SetError(HPRT_E_INVALID, f + ": n_lights is " + std::to_string(nLights) + ", the scene has " + std::to_string(s->dev.nLights) + " lights");
    if (p->max_depth > 1 && s->hasImageTexture && s->hasSpecularLobe)
        return SetError(HPRT_E_UNSUPPORTED, f + ": the scene holds an image texture and a material with a specular lobe; the reference carries ray differentials through "
                                            "SpecularReflect / SpecularTransmit (core/integrator.cpp:376-393, 416-445), which decide the texture's filter — not built");
    job->params = *p;
    job->nLightSamples.assign(nLights, 1);
    if (nLightSamples) job->nLightSamples.assign(nLightSamples, nLightSamples + nLights);
    return HPRT_OK;
}
int EnsureDlWorkspace(HprtScene *s, const DlJob &job, size_t nSlots, DlWorkspace *w) {
    const bool instances = s->dev.nInstances != 0u;
    const uint32_t nLights = (uint32_t)job.nLightSamples.size(), maxDepth = (uint32_t)job.params.max_depth;
    // ---- the per-light tables ----
    std::vector<uint32_t> first(nLights + 1, 0u); std::vector<uint2> itemLight;
    for (uint32_t j = 0; j < nLights; ++j) {
        first[j] = (uint32_t)itemLight.size();
        for (int32_t k = 0; k < job.nLightSamples[j]; ++k) itemLight.push_back(make_uint2(j, (uint32_t)k));
    }
    const uint32_t itemsPerHit = job.params.strategy == 1 ? 1u : (uint32_t)itemLight.size();
    if (itemLight.empty()) itemLight.push_back(make_uint2(0u, 0u));
    const size_t tA = ((nLights + 1) * 4 + 255) & ~(size_t)255, tB = tA;
    HIP_TRY(s->dlTables.alloc(tA + tB + itemLight.size() * sizeof(uint2) + 256));
    char *tb = s->dlTables.as<char>();
    if (nLights) {
        HIP_TRY(hipMemcpy(tb, job.nLightSamples.data(), nLights * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(tb + tA, first.data(), nLights * 4, hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMemcpy(tb + tA + tB, itemLight.data(), itemLight.size() * sizeof(uint2), hipMemcpyHostToDevice));
    w->dp.strategy = job.params.strategy; w->dp.maxDepth = job.params.max_depth; w->dp.nLights = nLights; w->dp.itemsPerHit = itemsPerHit;
    w->dp.arrayEndDim = 5 + (job.params.strategy == 0 ? 4 * (int32_t)maxDepth * (int32_t)nLights : 0);
    w->dp.nLightSamples = (const int32_t *)tb; w->dp.lightFirstItem = (const uint32_t *)(tb + tA); w->dp.itemLight = (const uint2 *)(tb + tA + tB);
    // ---- per camera sample ----
    const size_t perSlot = 4 + 16 * (size_t)DL_STACK_PLANES * maxDepth + 2 * 32 + 2 * 4 + 16 + (instances ? 8 : 0) + 16 * DL_RECORD_PLANES;
    HIP_TRY(s->dlSlots.alloc(nSlots * perSlot + 256 * 16));
    PlaneAllocator a{s->dlSlots.as<char>(), 0, 0};
    w->state.state = a.take<uint32_t>(nSlots);
    w->state.stack = a.take<float4>(nSlots * DL_STACK_PLANES * maxDepth); w->state.stride = (uint32_t)nSlots;
    for (int k = 0; k < 2; ++k) { w->node[k].a = a.take<float4>(nSlots); w->node[k].b = a.take<float4>(nSlots); w->live[k] = a.take<uint32_t>(nSlots); }
    w->hit.a = a.take<float4>(nSlots); w->hit.b = instances ? a.take<float2>(nSlots) : nullptr;
    w->recs.q = a.take<uint4>(nSlots); w->recs.tex = a.take<float4>(nSlots * (DL_RECORD_PLANES - 1)); w->recs.stride = (uint32_t)nSlots;
    w->counts = a.take<uint32_t>(256);
    // ---- per light sample: never less than one hit's items, never more than a step can produce ----
    const uint64_t most = std::max<uint64_t>((uint64_t)nSlots * std::max(1u, itemsPerHit), 1);
    w->itemCap = (size_t)std::min<uint64_t>(std::max<uint64_t>(g_dlRayCapacity, std::max(1u, itemsPerHit)), most);
    const size_t perItem = 2 * 16 + 4 + 32 + 1 + 32 + 16 + (instances ? 8 : 0);
    HIP_TRY(s->dlRays.alloc(w->itemCap * perItem + 256 * 16));
    PlaneAllocator b{s->dlRays.as<char>(), 0, 0};
    w->items.a = b.take<float4>(w->itemCap); w->items.b = b.take<float4>(w->itemCap); w->items.light = b.take<uint32_t>(w->itemCap);
    w->rays.shadow.a = b.take<float4>(w->itemCap); w->rays.shadow.b = b.take<float4>(w->itemCap); w->rays.occ = b.take<uint8_t>(w->itemCap);
    w->rays.bsdf.a = b.take<float4>(w->itemCap); w->rays.bsdf.b = b.take<float4>(w->itemCap);
    w->rays.bsdfHit.a = b.take<float4>(w->itemCap); w->rays.bsdfHit.b = instances ? b.take<float2>(w->itemCap) : nullptr;
    w->rays.shadowCount = w->counts + 64; w->rays.bsdfCount = w->counts + 128;
    return HPRT_OK;
}
// One batch of nSlots camera samples: k_generate, then step by step (one tree node per live sample) closest-hit trace -> k_dl_shade ->
// [hit count to the host] -> per range of hits whose light work fits the buffer: k_dl_rays -> [ray counts to the host] -> any-hit trace,
// closest-hit trace -> k_dl_resolve; then k_dl_advance -> [live count to the host].  Both traces are the scene's walk whatever the
// scene: these shadow rays could take the shadow grid (they end at a light), and do not — a follow-up.
int RunDlBatch(HprtScene *s, hipStream_t st, const RenderParams &rp, const DlWorkspace &w, const DlSlots &sl, uint32_t s0, uint32_t nSlots, bool count,
               const DlRadiance &out, EventTimer &ev, BatchTimers *bt, HprtRenderStats *stats, const IrregularSink *irregular) {
    PathStream camPath; camPath.ray = w.node[0]; camPath.beta = nullptr; camPath.L = nullptr;      // (k_generate stores the ray alone)
    DevCounters *ctr = s->counters.as<DevCounters>();
    uint32_t *wc = s->workCounter.as<uint32_t>();
    std::vector<std::pair<hipEvent_t, hipEvent_t>> evExt, evOcc, evDl[4];      // (evDl: the four kernels of device/direct.hip, for tools/bench_direct.py)
    auto timed = [&](std::vector<std::pair<hipEvent_t, hipEvent_t>> &into, auto launch) -> int {
        hipEvent_t e0 = ev.get(), e1 = ev.get();
        HIP_TRY(hipEventRecord(e0, st));
        launch();
        HIP_TRY(hipEventRecord(e1, st));
        into.push_back({e0, e1});
        return HPRT_OK;
    };
    auto flush = [&]() {
        for (auto &p : evExt) { float ms = 0; if (hipEventElapsedTime(&ms, p.first, p.second) == hipSuccess) bt->extendMs += ms; }
        for (auto &p : evOcc) { float ms = 0; if (hipEventElapsedTime(&ms, p.first, p.second) == hipSuccess) bt->occludedMs += ms; }
        for (int k = 0; k < 4; ++k) {
            for (auto &p : evDl[k]) { float ms = 0; if (hipEventElapsedTime(&ms, p.first, p.second) == hipSuccess) s->dlKernelMs[k] += ms; }
            evDl[k].clear();
        }
        evExt.clear(); evOcc.clear();
        ev.reset();
    };
    LaunchGenerate(st, s->dev, rp, camPath, s0, nSlots, irregular);
    uint32_t nLive = nSlots;
    const uint32_t *live = nullptr;      // step 0: node i is slot i
    const uint64_t maxSteps = ((uint64_t)1 << w.dp.maxDepth) - 1;
    for (uint64_t step = 0; nLive > 0; ++step) {
        if (step >= maxSteps) return SetError(HPRT_E_DEVICE, "internal error: a direct-lighting tree has more nodes than a full one");
        const int cur = (int)(step & 1);
        if (int rc = timed(evExt, [&] { Trace(s, st, false, count, nullptr, nullptr, nLive, nLive, w.node[cur], w.hit, nullptr, ctr, wc); })) return rc;
        bt->extendRays += nLive; ++bt->extendLaunches;
        stats->rays += nLive;
        HIP_TRY(hipMemsetAsync(w.counts, 0, 256 * sizeof(uint32_t), st));
        if (int rc = timed(evDl[0], [&] { LaunchDlShade(st, s->dev, rp, w.dp, sl, w.node[cur], w.hit, live, nLive, step == 0, w.state, w.recs, w.counts); })) return rc;
        HIP_TRY(hipMemcpyAsync(s->hostCounts + 9, w.counts, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const uint32_t nHits = s->hostCounts[9];
        if (nHits > nLive) return SetError(HPRT_E_DEVICE, "internal error: more direct-lighting hits than nodes");
        const uint32_t hitsPerRange = (uint32_t)(w.itemCap / std::max(1u, w.dp.itemsPerHit));
        for (uint32_t h0 = 0; h0 < nHits && w.dp.itemsPerHit; h0 += hitsPerRange) {
            const uint32_t nh = std::min(hitsPerRange, nHits - h0);
            HIP_TRY(hipMemsetAsync(w.counts + 64, 0, 128 * sizeof(uint32_t), st));
            if (int rc = timed(evDl[1], [&] { LaunchDlRays(st, s->dev, rp, w.dp, sl, w.state, w.recs, h0, nh, w.items, w.rays); })) return rc;
            HIP_TRY(hipMemcpyAsync(s->hostCounts + 10, w.rays.shadowCount, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(s->hostCounts + 11, w.rays.bsdfCount, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            const uint32_t nShadow = s->hostCounts[10], nBsdf = s->hostCounts[11];
            if (nShadow > w.itemCap || nBsdf > w.itemCap) return SetError(HPRT_E_DEVICE, "internal error: more direct-lighting rays than light samples");
            HitStream none; none.a = nullptr; none.b = nullptr;
            if (nShadow) {
                if (int rc = timed(evOcc, [&] { Trace(s, st, true, count, nullptr, nullptr, nShadow, nShadow, w.rays.shadow, none, w.rays.occ, ctr, wc); })) return rc;
                bt->occludedRays += nShadow; ++bt->occludedLaunches;
                stats->shadow_rays += nShadow;
            }
            if (nBsdf) {
                if (int rc = timed(evExt, [&] { Trace(s, st, false, count, nullptr, nullptr, nBsdf, nBsdf, w.rays.bsdf, w.rays.bsdfHit, nullptr, ctr, wc); })) return rc;
                bt->extendRays += nBsdf; ++bt->extendLaunches;
                stats->rays += nBsdf;
            }
            if (int rc = timed(evDl[2], [&] { LaunchDlResolve(st, s->dev, w.dp, w.state, w.recs, h0, nh, w.items, w.rays); })) return rc;
        }
        if (int rc = timed(evDl[3], [&] { LaunchDlAdvance(st, s->dev, rp, w.dp, sl, live, nLive, w.state, w.node[cur ^ 1], w.live[cur ^ 1], w.counts + 192, out); })) return rc;
        HIP_TRY(hipMemcpyAsync(s->hostCounts + 9, w.counts + 192, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
        const uint32_t nNext = s->hostCounts[9];
        if (nNext > nLive) return SetError(HPRT_E_DEVICE, "internal error: more direct-lighting children than nodes");
        flush();
        nLive = nNext; live = w.live[cur ^ 1];
        ++s->dlSteps;
    }
    return HPRT_OK;
}

}  // namespace

// SamplerIntegrator::Render (core/integrator.cpp:230-360) with the estimator of hprt_render (ao == dl == null: PathIntegrator::Li), of
// hprt_render_ao (AOIntegrator::Li) or of hprt_render_direct (DirectLightingIntegrator::Li): the same tiles, batches of camera samples,
// per-sample radiance store and film kernels
static int RenderImpl(HprtScene *s, const HprtRenderDesc *desc, const HprtAoParams *ao, float *d_film_xyzw, void *stream, HprtRenderStats *stats,
                      const DlJob *dl = nullptr) {
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    SceneCall call(s, st);      // (blocking: every path out of a started render has synchronised `st`, or failed)
    const HprtRenderOptions &o = desc->opt;
    int rc0;
    if (!ao && !dl) {
        if (o.spp <= 0 || o.max_depth < 0) return SetError(HPRT_E_INVALID, "spp must be positive and max_depth non-negative");
        if ((rc0 = CheckDepth(o.max_depth)) != HPRT_OK) return rc0;
    }
    FrameSetup f;
    int rc = SetupFrame(o, &f);
    if (rc != HPRT_OK) return rc;
    HprtRenderStats localStats; if (!stats) stats = &localStats;
    memset(stats, 0, sizeof(*stats));
    // ---- local tiles ----
    const int nTiles = f.ntx * f.nty;
    int tb = std::max(0, desc->tile_begin), te = desc->tile_end <= 0 ? nTiles : std::min(desc->tile_end, nTiles), ts = std::max(1, desc->tile_stride);
    f.localIndex.assign((size_t)f.W * f.H, -1);
    f.pixelXY.reserve((size_t)f.W * f.H / (size_t)ts + 256); f.pixelOffset.reserve((size_t)f.W * f.H / (size_t)ts + 256);
    std::vector<uint8_t> tileIsLocal(nTiles, 0);
    for (int t = tb; t < te; t += ts) { tileIsLocal[t] = 1; AddTilePixels(&f, t); }
    const uint32_t nPix = (uint32_t)f.pixelXY.size();
    const uint32_t spp = (uint32_t)o.spp;
    s->filmPixels = (size_t)f.W * f.H;
    s->filmW = f.W; s->filmH = f.H;
    s->nForeignRecords = 0; s->foreignExported = (desc->flags & HPRT_RENDER_EXPORT_FOREIGN) != 0;
    float *film = d_film_xyzw;
    if (!film) { HIP_TRY(s->film.alloc(16 * s->filmPixels)); film = s->film.as<float>(); }
    s->lastFilm = film;
    HIP_TRY(hipMemsetAsync(film, 0, 16 * s->filmPixels, st));
    if (nPix == 0) { HIP_TRY(hipStreamSynchronize(st)); return HPRT_OK; }
    // ---- sizes ----
    const size_t lallBytes = 3ull * spp * nPix * sizeof(float);
    if (lallBytes > (96ull << 30)) return SetError(HPRT_E_UNSUPPORTED, "per-sample radiance store would exceed 96 GiB; render in several tile ranges");
    // Paths per wavefront batch.  Every launch ends with a tail of half-empty waves and every bounce with a host
    // read-back, so batches are as large as memory allows: up to 256 M paths (365 B per path of streams and queues = 98 GB of the 288 GB;
    // 381 B with object instances), less if the device has less free (half of what is free now), and of EQUAL size (1,024 spp of the atrium:
    // two batches of 512 instead of 522 + 502 or, at the old 128 M cap, four of 256: -1 % per frame).  killeroo-simple
    // at 256 spp is one batch of 125 M paths: 6.5 % faster than two batches of 64 M.  (HPRT_BATCH_MPATHS changes the cap.)
    uint32_t chunk = 0;
    Workspace ps; QueueSet qa, qb; BinSet bins; AoWorkspace aw; DlWorkspace dw;
    if (dl) {
        for (double &ms : s->dlKernelMs) ms = 0;
        s->dlSteps = 0;
        // Direct lighting: spp_chunk keeps its meaning; left to the library, a batch holds up to kDlSlotCapacity camera samples, whose
        // light work goes through the ray buffer range by range (RunDlBatch)
        chunk = desc->spp_chunk > 0 ? (uint32_t)desc->spp_chunk : std::max<uint32_t>(1u, (uint32_t)(kDlSlotCapacity / nPix));
        chunk = std::min(chunk, spp);
        if ((uint64_t)chunk * nPix > 0x3fffffffull) chunk = std::max<uint32_t>(1u, (uint32_t)(0x3fffffffull / nPix));
        if ((rc = EnsureDlWorkspace(s, *dl, (size_t)chunk * nPix, &dw)) != HPRT_OK) return rc;
    } else if (ao) {
        for (double &ms : s->aoKernelMs) ms = 0;
        // Ambient occlusion: spp_chunk keeps its meaning, an upper bound per pixel; left to the library, a batch holds up to
        // kAoSlotCapacity camera samples.  Its hemisphere rays go through the ray buffer range by range (RunAoBatch).
        chunk = desc->spp_chunk > 0 ? (uint32_t)desc->spp_chunk : std::max<uint32_t>(1u, (uint32_t)(kAoSlotCapacity / nPix));
        chunk = std::min(chunk, spp);
        if ((uint64_t)chunk * nPix > 0x7fffffffull) chunk = (uint32_t)(0x7fffffffull / nPix);
        if ((rc = EnsureAoWorkspace(s, (size_t)chunk * nPix, (uint32_t)ao->n_samples, (uint64_t)chunk * nPix * (uint64_t)ao->n_samples, &aw)) != HPRT_OK) return rc;
    } else if ((rc = ChooseBatch(s, desc->spp_chunk, nPix, spp, &chunk)) != HPRT_OK) return rc;
    const size_t maxSlots = (size_t)chunk * nPix;
    if (!ao && !dl && (rc = EnsureWorkspace(s, maxSlots, &ps, &qa, &qb, &bins)) != HPRT_OK) return rc;
    HIP_TRY(s->Lall.alloc(lallBytes));
    if ((rc = PoisonWorkspace(s)) != HPRT_OK) return rc;
    float *LallR = s->Lall.as<float>(), *LallG = LallR + (size_t)spp * nPix, *LallB = LallG + (size_t)spp * nPix;
    HIP_TRY(upload(s->pixelXY, f.pixelXY)); HIP_TRY(upload(s->pixelOffset, f.pixelOffset));
    RenderParams rp;
    MakeCamera(o, &rp.cam);
    rp.hal.baseScale1 = f.hal.baseScales[1]; rp.hal.baseExp0 = f.hal.baseExponents[0]; rp.hal.sampleStride = f.hal.sampleStride;
    rp.hal.samplePixelCenter = o.sample_pixel_center;
    rp.pixelXY = s->pixelXY.as<uint32_t>(); rp.pixelOffset = s->pixelOffset.as<uint64_t>(); rp.nPix = nPix;
    rp.maxDepth = o.max_depth; rp.rrThreshold = o.rr_threshold;
    rp.invSqrtSpp = 1 / std::sqrt((float)spp);      // ScaleDifferentials' factor, core/integrator.cpp:288-289
    const bool wantPixelStats = (desc->flags & HPRT_RENDER_PIXEL_STATS) != 0;
    const bool count = (desc->flags & HPRT_RENDER_COUNT_WORK) != 0 || wantPixelStats;
    // a counting render traces exactly the reference's rays (its counters are the reference's) unless asked to count what a plain render traces
    rp.speculate = rp.foldRepair = 0;      // (RunBatch decides, batch by batch)
    rp.cullMis = (!count || (desc->flags & HPRT_RENDER_COUNT_TRACED) != 0) && !(desc->flags & HPRT_RENDER_TRACE_ALL) ? 1 : 0;
    uint32_t *pixelStats = nullptr;
    if (wantPixelStats) {
        HIP_TRY(s->rayStats.alloc(sizeof(uint4) * maxSlots));
        HIP_TRY(s->pixelStatsLocal.alloc(6ull * nPix * sizeof(uint32_t)));
        HIP_TRY(hipMemsetAsync(s->pixelStatsLocal.p, 0, 6ull * nPix * sizeof(uint32_t), st));
        HIP_TRY(s->pixelStatsFilm.alloc(7ull * s->filmPixels * sizeof(uint64_t)));
        HIP_TRY(hipMemsetAsync(s->pixelStatsFilm.p, 0, 7ull * s->filmPixels * sizeof(uint64_t), st));
        pixelStats = s->pixelStatsLocal.as<uint32_t>();
        if (CountsKdShare(s)) {
            HIP_TRY(s->pixelKdLocal.alloc(2ull * nPix * sizeof(uint32_t)));
            HIP_TRY(hipMemsetAsync(s->pixelKdLocal.p, 0, 2ull * nPix * sizeof(uint32_t), st));
            HIP_TRY(s->pixelKdFilm.alloc(2ull * s->filmPixels * sizeof(uint64_t)));
            HIP_TRY(hipMemsetAsync(s->pixelKdFilm.p, 0, 2ull * s->filmPixels * sizeof(uint64_t), st));
        }
    }
    s->pixelStatsValid = false; s->pixelKdValid = false;
    HIP_TRY(hipMemsetAsync(s->counters.p, 0, sizeof(DevCounters), st));
    if (CountsKdShare(s)) HIP_TRY(hipMemsetAsync(s->kdShare.p, 0, 2 * sizeof(unsigned long long), st));

    auto wall0 = std::chrono::high_resolution_clock::now();
    // ---- film footprint pre-pass ----
    // Irregular film samples: k_generate lists them while it forms the camera samples (capacity: a first guess — a few samples per
    // pixel have a zero Halton offset); if the guess was too small, k_find_irregular recounts with the counted size
    // (HPRT_IRREGULAR_CAP: test hook for that fallback)
    static const uint32_t capHint = [] { const char *e = getenv("HPRT_IRREGULAR_CAP"); return e ? (uint32_t)std::max(1, atoi(e)) : (1u << 24); }();
    uint32_t irrCap = (uint32_t)std::min<uint64_t>((uint64_t)nPix * spp, capHint);
    HIP_TRY(s->irregularCount.alloc(16));
    HIP_TRY(s->irregular.alloc((size_t)irrCap * sizeof(IrregularSample)));
    HIP_TRY(hipMemsetAsync(s->irregularCount.p, 0, 16, st));
    const IrregularSink sink = {f.fg, s->irregularCount.as<uint32_t>(), irrCap, s->irregular.as<IrregularSample>()};
    // ---- batches ----
    EventTimer ev; BatchTimers bt;
    for (uint32_t s0 = 0; s0 < spp; s0 += chunk) {
        const uint32_t c = std::min(chunk, spp - s0), nSlots = c * nPix;
        if (dl) {      // (k_dl_advance stores each sample where k_store_radiance would)
            rc = RunDlBatch(s, st, rp, dw, DlSlots{rp.pixelOffset, nullptr, nPix, s0}, s0, nSlots, count, DlRadiance{LallR, LallG, LallB, (size_t)s0 * nPix}, ev, &bt, stats, &sink);
            if (rc != HPRT_OK) return rc;
            continue;
        }
        if (ao) {      // (k_ao_frame and k_ao_resolve store each sample where k_store_radiance would)
            rc = RunAoBatch(s, st, rp, *ao, aw, nullptr, s0, nSlots, count, AoRadiance{LallR, LallG, LallB, (size_t)s0 * nPix}, ev, &bt, stats, &sink);
            if (rc != HPRT_OK) return rc;
            continue;
        }
        rc = RunBatch(s, st, rp, ps, qa, qb, bins, s0, nSlots, count, ev, &bt, stats, pixelStats, &sink);
        if (rc != HPRT_OK) return rc;
        LaunchStoreRadiance(st, ps.Lfinal, LallR, LallG, LallB, nPix, s0, nSlots);
    }
    HIP_TRY(hipMemcpyAsync(s->hostCounts + 8, s->irregularCount.p, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    uint32_t nIrr = s->hostCounts[8];
    if (nIrr > irrCap) {      // the list overflowed: once more, standalone, with room for all of them
        if ((uint64_t)nIrr * sizeof(IrregularSample) > (8ull << 30)) return SetError(HPRT_E_UNSUPPORTED, "too many irregular film samples");
        irrCap = nIrr;
        HIP_TRY(s->irregular.alloc((size_t)irrCap * sizeof(IrregularSample)));
        HIP_TRY(hipMemsetAsync(s->irregularCount.p, 0, 16, st));
        LaunchFindIrregular(st, s->dev, rp, f.fg, spp, s->irregularCount.as<uint32_t>(), irrCap, s->irregular.as<IrregularSample>());
        HIP_TRY(hipMemcpyAsync(s->hostCounts + 8, s->irregularCount.p, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (s->hostCounts[8] != nIrr) return SetError(HPRT_E_DEVICE, "internal error: irregular film samples counted differently");
    }
    std::vector<IrregularSample> irr(nIrr);
    if (nIrr) HIP_TRY(hipMemcpy(irr.data(), s->irregular.p, (size_t)nIrr * sizeof(IrregularSample), hipMemcpyDeviceToHost));
    std::vector<ExtraEntry> own, foreign;
    for (const IrregularSample &r : irr) {
        const uint32_t pxy = f.pixelXY[r.pix];
        const int qx = (int)(pxy & 0xffffu), qy = (int)(pxy >> 16);
        const int qtx = (qx - f.fg.sx0) / 16, qty = (qy - f.fg.sy0) / 16;
        const uint32_t qTile = (uint32_t)(qty * f.ntx + qtx);
        const uint32_t qPos = (uint32_t)((qy - (f.fg.sy0 + qty * 16)) * 16 + (qx - (f.fg.sx0 + qtx * 16)));
        for (int y = r.y0; y < r.y1; ++y)
            for (int x = r.x0; x < r.x1; ++x) {
                if (x == qx && y == qy) continue;
                const int dtx = (x - f.fg.sx0) / 16, dty = (y - f.fg.sy0) / 16;
                const uint32_t filmIdx = (uint32_t)((size_t)(y - f.fg.cy0) * f.W + (x - f.fg.cx0));
                ExtraEntry e; e.srcTile = qTile; e.srcPos = qPos; e.sample = r.sample; e.srcPix = r.pix;
                if (dtx == qtx && dty == qty) {
                    e.dest = (uint32_t)f.localIndex[filmIdx];
                    e.pre = (qy < y || (qy == y && qx < x)) ? 1 : 0;
                    own.push_back(e);
                } else { e.dest = filmIdx; e.pre = 0; foreign.push_back(e); }
            }
    }
    std::sort(own.begin(), own.end(), [](const ExtraEntry &a, const ExtraEntry &b) {
        if (a.dest != b.dest) return a.dest < b.dest;
        if (a.srcPos != b.srcPos) return a.srcPos < b.srcPos;   // pre entries have smaller positions than the destination's
        return a.sample < b.sample;
    });
    std::sort(foreign.begin(), foreign.end(), [](const ExtraEntry &a, const ExtraEntry &b) {
        if (a.dest != b.dest) return a.dest < b.dest;
        if (a.srcTile != b.srcTile) return a.srcTile < b.srcTile;
        if (a.srcPos != b.srcPos) return a.srcPos < b.srcPos;
        return a.sample < b.sample;
    });
    FilmExtras ex; memset(&ex, 0, sizeof(ex));
    std::vector<uint32_t> groupDest, groupTile;      // per foreign group (destination film pixel, source tile), sorted by both
    {
        std::vector<uint32_t> begin(nPix + 1, 0), src(own.size()), smp(own.size()); std::vector<uint8_t> pre(own.size());
        for (const ExtraEntry &e : own) ++begin[e.dest + 1];
        for (uint32_t i = 0; i < nPix; ++i) begin[i + 1] += begin[i];
        for (size_t i = 0; i < own.size(); ++i) { src[i] = own[i].srcPix; smp[i] = own[i].sample; pre[i] = own[i].pre; }
        HIP_TRY(upload(s->exOwnBegin, begin)); HIP_TRY(upload(s->exOwnSrc, src)); HIP_TRY(upload(s->exOwnSample, smp)); HIP_TRY(upload(s->exOwnPre, pre));
        ex.ownBegin = s->exOwnBegin.as<uint32_t>(); ex.ownSrcPix = s->exOwnSrc.as<uint32_t>(); ex.ownSample = s->exOwnSample.as<uint32_t>(); ex.ownIsPre = s->exOwnPre.as<uint8_t>();
        std::vector<uint32_t> dest, destBegin, groupBegin, fsrc(foreign.size()), fsmp(foreign.size());
        for (size_t i = 0; i < foreign.size(); ++i) {
            const bool newDest = i == 0 || foreign[i].dest != foreign[i - 1].dest;
            const bool newGroup = newDest || foreign[i].srcTile != foreign[i - 1].srcTile;
            if (newDest) { dest.push_back(foreign[i].dest); destBegin.push_back((uint32_t)groupBegin.size()); }
            if (newGroup) { groupBegin.push_back((uint32_t)i); groupDest.push_back(foreign[i].dest); groupTile.push_back(foreign[i].srcTile); }
            fsrc[i] = foreign[i].srcPix; fsmp[i] = foreign[i].sample;
        }
        destBegin.push_back((uint32_t)groupBegin.size()); groupBegin.push_back((uint32_t)foreign.size());
        HIP_TRY(upload(s->exFDest, dest)); HIP_TRY(upload(s->exFDestBegin, destBegin)); HIP_TRY(upload(s->exFGroupBegin, groupBegin));
        HIP_TRY(upload(s->exFSrc, fsrc)); HIP_TRY(upload(s->exFSample, fsmp));
        ex.nForeignDest = (uint32_t)dest.size();
        ex.foreignDestFilmIndex = s->exFDest.as<uint32_t>(); ex.foreignDestBegin = s->exFDestBegin.as<uint32_t>(); ex.foreignGroupBegin = s->exFGroupBegin.as<uint32_t>();
        ex.foreignSrcPix = s->exFSrc.as<uint32_t>(); ex.foreignSample = s->exFSample.as<uint32_t>();
    }
    LaunchFilmOwn(st, rp, f.fg, LallR, LallG, LallB, spp, ex, film);
    if (desc->flags & HPRT_RENDER_EXPORT_FOREIGN) {
        // cross-tile contributions leave as records: hprt_film_gather merges those of all ranks in source-tile order
        const uint32_t nGroups = (uint32_t)groupDest.size();
        HIP_TRY(upload(s->exGroupDest, groupDest)); HIP_TRY(upload(s->exGroupTile, groupTile));
        HIP_TRY(s->foreignRecords.alloc(std::max<size_t>(1, nGroups) * sizeof(FilmRecord)));
        LaunchFilmForeignExport(st, rp, f.fg, LallR, LallG, LallB, ex, nGroups, s->exGroupDest.as<uint32_t>(), s->exGroupTile.as<uint32_t>(),
                                s->foreignRecords.as<FilmRecord>());
        s->nForeignRecords = nGroups;
    } else
        LaunchFilmForeign(st, rp, f.fg, LallR, LallG, LallB, ex, film);
    if (pixelStats) {
        LaunchPixelStatsToFilm(st, pixelStats, rp.pixelXY, nPix, spp, f.fg.cx0, f.fg.cy0, f.W, s->pixelStatsFilm.as<unsigned long long>());
        s->pixelStatsValid = true;
        if (CountsKdShare(s)) {
            LaunchPixelKdStatsToFilm(st, s->pixelKdLocal.as<uint32_t>(), rp.pixelXY, nPix, f.fg.cx0, f.fg.cy0, f.W, s->filmPixels,
                                     s->pixelKdFilm.as<unsigned long long>());
            s->pixelKdValid = true;
        }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    stats->render_seconds = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - wall0).count();
    stats->camera_rays = (uint64_t)nPix * spp;
    stats->extend_seconds = bt.extendMs * 1e-3; stats->occluded_seconds = bt.occludedMs * 1e-3;
    stats->extend_launches = bt.extendLaunches; stats->occluded_launches = bt.occludedLaunches;
    stats->extend_rays = bt.extendRays; stats->occluded_rays = bt.occludedRays;
    if (count) {
        DevCounters c;
        HIP_TRY(hipMemcpy(&c, s->counters.p, sizeof(c), hipMemcpyDeviceToHost));
        stats->nodes_fetched = c.nodesFetched; stats->nodes_entered = c.nodesEntered; stats->tri_tests = c.triTests; stats->sphere_tests = c.sphereTests;
        stats->nodes_fetched_p = c.nodesFetchedP; stats->nodes_entered_p = c.nodesEnteredP; stats->tri_tests_p = c.triTestsP; stats->sphere_tests_p = c.sphereTestsP;
    }
    return HPRT_OK;
}
int hprt_render(HprtScene *s, const HprtRenderDesc *desc, float *d_film_xyzw, void *stream, HprtRenderStats *stats) try {
    if (!s || !desc) return SetError(HPRT_E_INVALID, "hprt_render: null argument");
    return RenderImpl(s, desc, nullptr, d_film_xyzw, stream, stats);
} catch (...) { return hprt::HandleException(); }
// The parameters are judged before the scene and the device are looked at: a refusal does not depend on either
int hprt_render_ao(HprtScene *s, const HprtRenderDesc *desc, const HprtAoParams *ao, float *d_film_xyzw, void *stream, HprtRenderStats *stats) try {
    if (!desc) return SetError(HPRT_E_INVALID, "hprt_render_ao: null argument");
    if (int rc = CheckAoParams(ao, desc->opt.spp, "hprt_render_ao")) return rc;
    if (desc->flags & ~HPRT_RENDER_COUNT_WORK)
        return SetError(HPRT_E_UNSUPPORTED, "hprt_render_ao: only HPRT_RENDER_COUNT_WORK is supported (per-pixel statistics, EXPORT_FOREIGN, TRACE_ALL and "
                                            "COUNT_TRACED stay with hprt_render)");
    int dev;
    if (int rc = CheckDevice(s ? s->device : -1, &dev)) return rc;
    if (!s) return SetError(HPRT_E_INVALID, "hprt_render_ao: null argument");
    return RenderImpl(s, desc, ao, d_film_xyzw, stream, stats);
} catch (...) { return hprt::HandleException(); }
// Diagnostics hook (not part of include/hprt.h; tools/bench_ao.py): HIP-event seconds of k_ao_frame, k_ao_rays and k_ao_resolve in the
// scene's last hprt_render_ao
__attribute__((visibility("default"))) int hprt_debug_ao_kernel_seconds(HprtScene *s, double out3[3]) {
    if (!s || !out3) return HPRT_E_INVALID;
    for (int k = 0; k < 3; ++k) out3[k] = s->aoKernelMs[k] * 1e-3;
    return HPRT_OK;
}
// Diagnostics hook (not part of include/hprt.h; tests/test_gpu_ao.py): the hemisphere rays one any-hit launch of later hprt_render_ao
// calls takes at most (never fewer than one hit's); 0: back to the default.  Returns the setting before.
__attribute__((visibility("default"))) size_t hprt_debug_ao_ray_capacity(size_t rays) {
    const size_t was = g_aoRayCapacity;
    g_aoRayCapacity = rays ? rays : kAoRayCapacity;
    return was;
}

// The parameters and the scene's host-side facts are judged before the device is looked at: a refusal does not depend on it
int hprt_render_direct(HprtScene *s, const HprtRenderDesc *desc, const HprtDirectParams *params, const int32_t *n_light_samples, size_t n_lights,
                       float *d_film_xyzw, void *stream, HprtRenderStats *stats) try {
    if (!desc) return SetError(HPRT_E_INVALID, "hprt_render_direct: null argument");
    DlJob job;
    if (int rc = CheckDirect(s, params, n_light_samples, n_lights, desc->opt.spp, desc->flags, "hprt_render_direct", &job)) return rc;
    int dev;
    if (int rc = CheckDevice(s->device, &dev)) return rc;
    return RenderImpl(s, desc, nullptr, d_film_xyzw, stream, stats, &job);
} catch (...) { return hprt::HandleException(); }
// Diagnostics hook (not part of include/hprt.h; tools/bench_direct.py): HIP-event seconds of k_dl_shade, k_dl_rays, k_dl_resolve and
// k_dl_advance in the scene's last hprt_render_direct, and the tree-walk steps its batches took
__attribute__((visibility("default"))) int hprt_debug_dl_kernel_seconds(HprtScene *s, double out5[5]) {
    if (!s || !out5) return HPRT_E_INVALID;
    for (int k = 0; k < 4; ++k) out5[k] = s->dlKernelMs[k] * 1e-3;
    out5[4] = (double)s->dlSteps;
    return HPRT_OK;
}
// Diagnostics hook (not part of include/hprt.h; tests/test_gpu_direct.py): the light samples one pair of trace launches of later
// hprt_render_direct calls takes at most (never fewer than one hit's); 0: back to the default.  Returns the setting before.
__attribute__((visibility("default"))) size_t hprt_debug_dl_ray_capacity(size_t items) {
    const size_t was = g_dlRayCapacity;
    g_dlRayCapacity = items ? items : kDlRayCapacity;
    return was;
}

// Pays for the coming hprt_render(s, desc, ...) at load time: the wavefront workspace (path streams and queues: ~365 B per path of
// a batch, 98 GB for a 256 M-path batch) and the per-sample radiance store are allocated now, so that the render itself starts
// with its first kernel.  (A fresh process gets 100 GB in under a millisecond, but right after another process released as much the
// driver may spend seconds reclaiming it inside hipMalloc — DESIGN.md §7; a pbrt host renders once and would pay that inside Render().)
int hprt_scene_reserve(HprtScene *s, const HprtRenderDesc *desc) try {
    if (!s || !desc) return SetError(HPRT_E_INVALID, "hprt_scene_reserve: null argument");
    const HprtRenderOptions &o = desc->opt;
    if (o.spp <= 0 || o.max_depth < 0) return SetError(HPRT_E_INVALID, "spp must be positive and max_depth non-negative");
    HIP_TRY(hipSetDevice(s->device));
    SceneCall call(s, nullptr);
    FrameSetup f;
    int rc = SetupFrame(o, &f);
    if (rc != HPRT_OK) return rc;
    const int nTiles = f.ntx * f.nty;
    const int tb = std::max(0, desc->tile_begin), te = desc->tile_end <= 0 ? nTiles : std::min(desc->tile_end, nTiles), ts = std::max(1, desc->tile_stride);
    uint64_t nPix64 = 0;
    for (int t = tb; t < te; t += ts) {
        const int tx = t % f.ntx, ty = t / f.ntx;
        const int x0 = f.fg.sx0 + tx * 16, x1 = std::min(x0 + 16, f.fg.sx1), y0 = f.fg.sy0 + ty * 16, y1 = std::min(y0 + 16, f.fg.sy1);
        nPix64 += (uint64_t)(x1 - x0) * (uint64_t)(y1 - y0);
    }
    if (nPix64 == 0) return HPRT_OK;
    const uint32_t nPix = (uint32_t)nPix64, spp = (uint32_t)o.spp;
    const size_t lallBytes = 3ull * spp * nPix * sizeof(float);
    if (lallBytes > (96ull << 30)) return SetError(HPRT_E_UNSUPPORTED, "per-sample radiance store would exceed 96 GiB; render in several tile ranges");
    uint32_t chunk = 0;
    if ((rc = ChooseBatch(s, desc->spp_chunk, nPix, spp, &chunk)) != HPRT_OK) return rc;
    Workspace ps; QueueSet qa, qb; BinSet bins;
    if ((rc = EnsureWorkspace(s, (size_t)chunk * nPix, &ps, &qa, &qb, &bins)) != HPRT_OK) return rc;
    HIP_TRY(s->Lall.alloc(lallBytes));
    HIP_TRY(s->pixelXY.alloc((size_t)nPix * sizeof(uint32_t))); HIP_TRY(s->pixelOffset.alloc((size_t)nPix * sizeof(uint64_t)));
    HIP_TRY(hipDeviceSynchronize());
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }

// Pixel::stats of the last hprt_render with HPRT_RENDER_PIXEL_STATS (core/film.h:91): 7 values per film pixel
int hprt_pixel_stats_read(HprtScene *s, uint64_t *out7, size_t n_pixels) try {
    if (!s || !out7) return SetError(HPRT_E_INVALID, "hprt_pixel_stats_read: null argument");
    SceneCall call(s, nullptr);
    if (!s->pixelStatsValid) return SetError(HPRT_E_INVALID, "no per-pixel statistics: render with HPRT_RENDER_PIXEL_STATS first");
    if (n_pixels != s->filmPixels) return SetError(HPRT_E_INVALID, "hprt_pixel_stats_read: pixel count differs from the last render's film");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipMemcpy(out7, s->pixelStatsFilm.p, 7 * n_pixels * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
// the kd share of slots 5 / 6 of the last rbspkd or bsppaperkd render with HPRT_RENDER_PIXEL_STATS: [2][film pixels]
int hprt_pixel_kd_stats_read(HprtScene *s, uint64_t *out2, size_t n_pixels) try {
    if (!s || !out2) return SetError(HPRT_E_INVALID, "hprt_pixel_kd_stats_read: null argument");
    SceneCall call(s, nullptr);
    if (!s->pixelKdValid && (s->walk == HprtScene::Walk::RbspInst || s->walk == HprtScene::Walk::BspPaperInst) && s->pixelStatsValid) {      // plain two-level RBSP / general BSP trees: no node is a kd node
        if (n_pixels != s->filmPixels) return SetError(HPRT_E_INVALID, "hprt_pixel_kd_stats_read: pixel count differs from the last render's film");
        memset(out2, 0, 2 * n_pixels * sizeof(uint64_t));
        return HPRT_OK;
    }
    if (!s->pixelKdValid) return SetError(HPRT_E_INVALID, "no per-pixel kd statistics: render an rbspkd or bsppaperkd scene with HPRT_RENDER_PIXEL_STATS first");
    if (n_pixels != s->filmPixels) return SetError(HPRT_E_INVALID, "hprt_pixel_kd_stats_read: pixel count differs from the last render's film");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipMemcpy(out2, s->pixelKdFilm.p, 2 * n_pixels * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
int hprt_film_read(HprtScene *s, float *xyzw_out, size_t n_pixels) try {
    if (!s || !xyzw_out) return SetError(HPRT_E_INVALID, "hprt_film_read: null argument");
    SceneCall call(s, nullptr);
    if (!s->film.p || s->lastFilm != s->film.as<float>() || n_pixels != s->filmPixels)
        return SetError(HPRT_E_INVALID, "hprt_film_read: the last render did not write a library-owned film of that size (render with d_film_xyzw == NULL first)");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipMemcpy(xyzw_out, s->film.p, 16 * n_pixels, hipMemcpyDeviceToHost));
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }

int hprt_sample_radiance(HprtScene *s, const HprtRenderOptions *opt, size_t n, const int32_t *px, const int32_t *py, const int64_t *sample,
                         float *L_out) try {
    if (!s || !opt || (n && (!px || !py || !sample || !L_out))) return SetError(HPRT_E_INVALID, "hprt_sample_radiance: null argument");
    if (n == 0) return HPRT_OK;
    if (n > (1u << 26)) return SetError(HPRT_E_INVALID, "hprt_sample_radiance: too many samples in one call");
    if (opt->max_depth < 0) return SetError(HPRT_E_INVALID, "max_depth must be non-negative");
    if (int rcd = CheckDepth(opt->max_depth)) return rcd;
    HIP_TRY(hipSetDevice(s->device));
    SceneCall call(s, nullptr);
    FrameSetup f;
    int rc = SetupFrame(*opt, &f);
    if (rc != HPRT_OK) return rc;
    std::vector<uint32_t> xy(n); std::vector<uint64_t> off(n);
    for (size_t i = 0; i < n; ++i) {
        if (px[i] < f.fg.sx0 || px[i] >= f.fg.sx1 || py[i] < f.fg.sy0 || py[i] >= f.fg.sy1 || sample[i] < 0)
            return SetError(HPRT_E_INVALID, "hprt_sample_radiance: pixel outside the sample bounds");
        xy[i] = (uint32_t)px[i] | ((uint32_t)py[i] << 16);
        off[i] = (uint64_t)HaltonPixelOffset(f.hal, px[i], py[i]) + (uint64_t)sample[i] * (uint64_t)f.hal.sampleStride;
    }
    Workspace ps; QueueSet qa, qb; BinSet bins;
    rc = EnsureWorkspace(s, n, &ps, &qa, &qb, &bins);
    if (rc != HPRT_OK) return rc;
    HIP_TRY(upload(s->pixelXY, xy)); HIP_TRY(upload(s->pixelOffset, off));
    HIP_TRY(s->Lall.alloc(12 * n));
    if ((rc = PoisonWorkspace(s)) != HPRT_OK) return rc;
    RenderParams rp;
    MakeCamera(*opt, &rp.cam);
    rp.hal.baseScale1 = f.hal.baseScales[1]; rp.hal.baseExp0 = f.hal.baseExponents[0]; rp.hal.sampleStride = f.hal.sampleStride;
    rp.hal.samplePixelCenter = opt->sample_pixel_center;
    rp.pixelXY = s->pixelXY.as<uint32_t>(); rp.pixelOffset = s->pixelOffset.as<uint64_t>(); rp.nPix = (uint32_t)n;
    rp.maxDepth = opt->max_depth; rp.rrThreshold = opt->rr_threshold;
    rp.invSqrtSpp = 1 / std::sqrt((float)std::max(1, opt->spp)); rp.cullMis = 1; rp.speculate = rp.foldRepair = 0;      // (RunBatch decides)
    EventTimer ev; BatchTimers bt; HprtRenderStats stats; memset(&stats, 0, sizeof(stats));
    rc = RunBatch(s, nullptr, rp, ps, qa, qb, bins, 0, (uint32_t)n, false, ev, &bt, &stats);
    if (rc != HPRT_OK) return rc;
    float *LR = s->Lall.as<float>();
    LaunchStoreRadiance(nullptr, ps.Lfinal, LR, LR + n, LR + 2 * n, (uint32_t)n, 0, (uint32_t)n);
    HIP_TRY(hipGetLastError()); HIP_TRY(hipDeviceSynchronize());
    std::vector<float> planes(3 * n);
    HIP_TRY(hipMemcpy(planes.data(), LR, 12 * n, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) { L_out[3 * i] = planes[i]; L_out[3 * i + 1] = planes[n + i]; L_out[3 * i + 2] = planes[2 * n + i]; }
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }

// hprt_sample_radiance for the ambient-occlusion estimator: slot i is sample[i] of pixel (px[i], py[i]); its camera sample sits at
// GetIndexForSample(sample), its array samples at GetIndexForSample(sample * n_samples + j)
int hprt_sample_ao(HprtScene *s, const HprtRenderOptions *opt, const HprtAoParams *ao, size_t n, const int32_t *px, const int32_t *py,
                   const int64_t *sample, float *L3_out) try {
    if (!opt || (n && (!px || !py || !sample || !L3_out))) return SetError(HPRT_E_INVALID, "hprt_sample_ao: null argument");
    if (int rc = CheckAoParams(ao, std::max(1, opt->spp), "hprt_sample_ao")) return rc;
    if (n > (1u << 22)) return SetError(HPRT_E_INVALID, "hprt_sample_ao: too many samples in one call");
    int dev;
    if (int rc = CheckDevice(s ? s->device : -1, &dev)) return rc;
    if (!s) return SetError(HPRT_E_INVALID, "hprt_sample_ao: null argument");
    if (n == 0) return HPRT_OK;
    SceneCall call(s, nullptr);
    FrameSetup f;
    int rc = SetupFrame(*opt, &f);
    if (rc != HPRT_OK) return rc;
    std::vector<uint32_t> xy(n); std::vector<uint64_t> off(2 * n);      // camera-sample indices, then the first array sample's
    for (size_t i = 0; i < n; ++i) {
        if (px[i] < f.fg.sx0 || px[i] >= f.fg.sx1 || py[i] < f.fg.sy0 || py[i] >= f.fg.sy1 || sample[i] < 0 || sample[i] > 0x7fffffffll)
            return SetError(HPRT_E_INVALID, "hprt_sample_ao: pixel outside the sample bounds, or sample number out of range");
        xy[i] = (uint32_t)px[i] | ((uint32_t)py[i] << 16);
        const uint64_t pixelOffset = (uint64_t)HaltonPixelOffset(f.hal, px[i], py[i]);
        off[i] = pixelOffset + (uint64_t)sample[i] * (uint64_t)f.hal.sampleStride;
        off[n + i] = pixelOffset + (uint64_t)sample[i] * (uint64_t)ao->n_samples * (uint64_t)f.hal.sampleStride;
    }
    AoWorkspace aw;
    if ((rc = EnsureAoWorkspace(s, n, (uint32_t)ao->n_samples, (uint64_t)n * (uint64_t)ao->n_samples, &aw)) != HPRT_OK) return rc;
    HIP_TRY(upload(s->pixelXY, xy)); HIP_TRY(upload(s->pixelOffset, off));
    HIP_TRY(s->Lall.alloc(12 * n));
    if ((rc = PoisonWorkspace(s)) != HPRT_OK) return rc;
    RenderParams rp;
    MakeCamera(*opt, &rp.cam);
    rp.hal.baseScale1 = f.hal.baseScales[1]; rp.hal.baseExp0 = f.hal.baseExponents[0]; rp.hal.sampleStride = f.hal.sampleStride;
    rp.hal.samplePixelCenter = opt->sample_pixel_center;
    rp.pixelXY = s->pixelXY.as<uint32_t>(); rp.pixelOffset = s->pixelOffset.as<uint64_t>(); rp.nPix = (uint32_t)n;
    rp.maxDepth = 0; rp.rrThreshold = 0.f; rp.invSqrtSpp = 1.f; rp.cullMis = 1; rp.speculate = rp.foldRepair = 0;      // (not read)
    EventTimer ev; BatchTimers bt; HprtRenderStats stats; memset(&stats, 0, sizeof(stats));
    float *LR = s->Lall.as<float>();
    rc = RunAoBatch(s, nullptr, rp, *ao, aw, rp.pixelOffset + n, 0, (uint32_t)n, false, AoRadiance{LR, LR + n, LR + 2 * n, 0}, ev, &bt, &stats, nullptr);
    if (rc != HPRT_OK) return rc;
    HIP_TRY(hipGetLastError()); HIP_TRY(hipDeviceSynchronize());
    std::vector<float> planes(3 * n);
    HIP_TRY(hipMemcpy(planes.data(), LR, 12 * n, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) { L3_out[3 * i] = planes[i]; L3_out[3 * i + 1] = planes[n + i]; L3_out[3 * i + 2] = planes[2 * n + i]; }
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }

// hprt_sample_radiance for the direct-lighting estimator: slot i is sample[i] of pixel (px[i], py[i]); its camera sample and plain
// dimensions sit at GetIndexForSample(sample), element k of an array of size n at GetIndexForSample(sample * n + k)
int hprt_sample_direct(HprtScene *s, const HprtRenderOptions *opt, const HprtDirectParams *params, const int32_t *n_light_samples, size_t n_lights, size_t n,
                       const int32_t *px, const int32_t *py, const int64_t *sample, float *L3_out) try {
    if (!opt || (n && (!px || !py || !sample || !L3_out))) return SetError(HPRT_E_INVALID, "hprt_sample_direct: null argument");
    DlJob job;
    if (int rc = CheckDirect(s, params, n_light_samples, n_lights, std::max(1, opt->spp), 0, "hprt_sample_direct", &job)) return rc;
    if (n > (1u << 22)) return SetError(HPRT_E_INVALID, "hprt_sample_direct: too many samples in one call");
    int dev;
    if (int rc = CheckDevice(s->device, &dev)) return rc;
    if (n == 0) return HPRT_OK;
    SceneCall call(s, nullptr);
    FrameSetup f;
    int rc = SetupFrame(*opt, &f);
    if (rc != HPRT_OK) return rc;
    // camera-sample indices (k_generate's), then the pixels' own offsets; the sample numbers travel with the pixel words
    std::vector<uint32_t> xy(2 * n); std::vector<uint64_t> off(2 * n);
    for (size_t i = 0; i < n; ++i) {
        if (px[i] < f.fg.sx0 || px[i] >= f.fg.sx1 || py[i] < f.fg.sy0 || py[i] >= f.fg.sy1 || sample[i] < 0 || sample[i] > 0x7fffffffll)
            return SetError(HPRT_E_INVALID, "hprt_sample_direct: pixel outside the sample bounds, or sample number out of range");
        for (int32_t c : job.nLightSamples)
            if (job.params.strategy == 0 && (int64_t)c * (sample[i] + 1) > 0x7fffffffll)
                return SetError(HPRT_E_UNSUPPORTED, "hprt_sample_direct: a light's sample count * (sample + 1) exceeds INT32_MAX");
        xy[i] = (uint32_t)px[i] | ((uint32_t)py[i] << 16);
        xy[n + i] = (uint32_t)sample[i];
        const uint64_t pixelOffset = (uint64_t)HaltonPixelOffset(f.hal, px[i], py[i]);
        off[i] = pixelOffset + (uint64_t)sample[i] * (uint64_t)f.hal.sampleStride;
        off[n + i] = pixelOffset;
    }
    DlWorkspace dw;
    if ((rc = EnsureDlWorkspace(s, job, n, &dw)) != HPRT_OK) return rc;
    HIP_TRY(upload(s->pixelXY, xy)); HIP_TRY(upload(s->pixelOffset, off));
    HIP_TRY(s->Lall.alloc(12 * n));
    if ((rc = PoisonWorkspace(s)) != HPRT_OK) return rc;
    RenderParams rp;
    MakeCamera(*opt, &rp.cam);
    rp.hal.baseScale1 = f.hal.baseScales[1]; rp.hal.baseExp0 = f.hal.baseExponents[0]; rp.hal.sampleStride = f.hal.sampleStride;
    rp.hal.samplePixelCenter = opt->sample_pixel_center;
    rp.pixelXY = s->pixelXY.as<uint32_t>(); rp.pixelOffset = s->pixelOffset.as<uint64_t>(); rp.nPix = (uint32_t)n;
    rp.maxDepth = 0; rp.rrThreshold = 0.f; rp.cullMis = 1; rp.speculate = rp.foldRepair = 0;      // (not read)
    rp.invSqrtSpp = 1 / std::sqrt((float)std::max(1, opt->spp));      // ScaleDifferentials' factor, core/integrator.cpp:288-289
    EventTimer ev; BatchTimers bt; HprtRenderStats stats; memset(&stats, 0, sizeof(stats));
    float *LR = s->Lall.as<float>();
    // (the camera index of slot i is rp.pixelOffset[i] + 0 * stride: s0 = 0 and nPix = n make k_generate's sample number 0; the estimator
    // reads the pixel's own offset and the sample number)
    rc = RunDlBatch(s, nullptr, rp, dw, DlSlots{rp.pixelOffset + n, rp.pixelXY + n, (uint32_t)n, 0u}, 0, (uint32_t)n, false, DlRadiance{LR, LR + n, LR + 2 * n, 0}, ev, &bt,
                    &stats, nullptr);
    if (rc != HPRT_OK) return rc;
    HIP_TRY(hipGetLastError()); HIP_TRY(hipDeviceSynchronize());
    std::vector<float> planes(3 * n);
    HIP_TRY(hipMemcpy(planes.data(), LR, 12 * n, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) { L3_out[3 * i] = planes[i]; L3_out[3 * i + 1] = planes[n + i]; L3_out[3 * i + 2] = planes[2 * n + i]; }
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }

// Diagnostics hook (not part of include/hprt.h; host code only, no device needed): the Halton index of sample `sample[i]` at pixel
// (px[i], py[i]) of the frame `opt` describes, both ways the library forms it — via_tables: a render's, from SetupFrame's offX / offY
// tables (AddTilePixels); direct: hprt_sample_radiance's, from HaltonPixelOffset — and the frame's sample bounds {sx0, sy0, sx1, sy1}.
__attribute__((visibility("default"))) int hprt_debug_halton_index(const HprtRenderOptions *opt, size_t n, const int32_t *px, const int32_t *py, const int64_t *sample,
                                                                    uint64_t *via_tables, uint64_t *direct, int32_t *sample_bounds4) try {
    if (!opt || !sample_bounds4 || (n && (!px || !py || !sample || !via_tables || !direct))) return SetError(HPRT_E_INVALID, "hprt_debug_halton_index: null argument");
    FrameSetup f;
    if (int rc = SetupFrame(*opt, &f)) return rc;
    sample_bounds4[0] = f.fg.sx0; sample_bounds4[1] = f.fg.sy0; sample_bounds4[2] = f.fg.sx1; sample_bounds4[3] = f.fg.sy1;
    for (size_t i = 0; i < n; ++i) {
        if (px[i] < f.fg.sx0 || px[i] >= f.fg.sx1 || py[i] < f.fg.sy0 || py[i] >= f.fg.sy1 || sample[i] < 0)
            return SetError(HPRT_E_INVALID, "hprt_debug_halton_index: pixel outside the sample bounds");
        via_tables[i] = TilePixelOffset(f, px[i], py[i]) + (uint64_t)sample[i] * (uint64_t)f.hal.sampleStride;
        direct[i] = (uint64_t)HaltonPixelOffset(f.hal, px[i], py[i]) + (uint64_t)sample[i] * (uint64_t)f.hal.sampleStride;
    }
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }

}  // extern "C"
