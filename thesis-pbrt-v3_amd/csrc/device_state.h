// hprt — host-side state of a device scene, shared by capi_device.hip (upload, trace, render) and
// capi_gather.hip (multi-GPU film gather).  Library-internal.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <mutex>
#include <string>
#include <vector>
#include "../../include/hprt.h"
#include "device/kernels.h"
#include "device/kd_walk.h"
#include "device/rbsp_walk.h"
#include "device/rbspkd_walk.h"
#include "device/bsppaper_walk.h"
#include "device/bsppaperkd_walk.h"
#include "device/kdinst_walk.h"
#include "device/rbspinst_walk.h"
#include "device/bsppaperinst_walk.h"
#include "device/shadow_grid.h"
#include "device/distant_grid.h"
#include "hprt_internal.h"

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e__ = (expr);                                                                        \
        if (e__ != hipSuccess)                                                                          \
            return hprt::SetError(HPRT_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e__));   \
    } while (0)

namespace hprt {

struct DevBuf {
    void *p = nullptr; size_t bytes = 0;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n) {
        if (p && bytes >= n) return hipSuccess;
        if (p) { (void)hipFree(p); p = nullptr; bytes = 0; }
        if (n == 0) return hipSuccess;
        hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) bytes = n;
        return e;
    }
    template <typename T> T *as() const { return (T *)p; }
};
template <typename T> hipError_t upload(DevBuf &b, const std::vector<T> &v) {
    hipError_t e = b.alloc(std::max<size_t>(v.size() * sizeof(T), 16));
    if (e != hipSuccess || v.empty()) return e;
    return hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}

}  // namespace hprt

struct HprtScene;
namespace hprt {
// Scope of one call on a scene: takes the scene's mutex and orders the call's stream behind the last asynchronous call.
struct SceneCall {
    std::unique_lock<std::mutex> lk; HprtScene *s; hipStream_t st;
    SceneCall(HprtScene *scene, hipStream_t stream);
    void leave_async();      // the call returns with work still queued on `st`: later calls must wait for it
};
}  // namespace hprt

struct HprtScene {
    int device = 0;
    // One call in flight per scene (include/hprt.h "Concurrency"): the work counter, the stream copies of the *_device calls, the
    // deep-stack area and the render workspace belong to the scene, not to a call.  Host threads are serialised by `mu`; the
    // asynchronous *_device calls leave `lastUse` behind on their stream and every later call makes ITS stream wait for it, so
    // calls on different streams run one after the other on the device too.
    std::mutex mu;
    hipEvent_t lastUse = nullptr; bool lastUsePending = false;
    hprt::DevScene dev;
    hprt::DevBuf textures, mipLevels, texels, weightLut;
    hprt::DevBuf nodes, tris, primVtx, primN, vUV, vS, shapes, materials, lights, spheres, instances, topEntry, topEntryWide, lightFunc, lightCdf, perms, primes, primeSums, primeMagic;
    hprt::DevBuf envLights, envData;      // infinite lights: DevEnvLight table and their Distribution2D tables
    hprt::DevBuf wide, leafBox;           // the leaf-exact walk structure (wide_bvh.h)
    // the scene's shadow grid: the light-centred one of a point light (shadow_grid.h), the light-aligned one of a distant light
    // (distant_grid.h), or none (its shadow rays take the walk).  grid: the kernel's arguments, of which k_shadow_grid takes all but
    // the frame; gridInfo: what hprt_debug_{shadow,distant}_grid_info report.
    hprt::GridKind gridKind = hprt::GridKind::None;
    hprt::DevBuf gridImage; hprt::DevDistantGrid grid{};
    struct GridInfo { size_t nEntries = 0; uint32_t longest = 0; double buildSeconds = 0, packSeconds = 0, eps = 0; size_t bytes = 0; float light[3] = {0, 0, 0}; uint64_t renderLaunches = 0; } gridInfo;
    hprt::DevBuf counters, workCounter, deepStack;
    // hprt_debug_capture_rays (tools/sort_experiment.py): the next render copies the rays one bounce queues into a caller buffer
    struct Capture { int bounce = -1, kind = 0; float *out7 = nullptr; size_t cap = 0, n = 0; } capture;
    // hprt_debug_shade_counts (tests): while on, every bounce also reads how many vertices the specialised shading variants deferred to the
    // generic bin and how many waited in the retry lists; sums since it was switched on
    bool shadeCountsOn = false; uint64_t shadeDeferred = 0, shadeRetried = 0;
    // (the same switch) vertices whose light sample k_shade added at once, those of them k_repair set back, and full vertices (k_resolve)
    uint64_t shadeSpeculated = 0, shadeRepaired = 0, shadeFull = 0;
    int poisonByte = -1;      // hprt_debug_poison_workspace (tests): fill every stream, queue and stack with this byte before each render
    hprt::DevBuf voxFunc, voxCdf, voxFuncInt, voxRi;      // SpatialLightDistribution tables (lightsamplestrategy "spatial")
    hprt::DevBuf voxSlot, voxRequest, voxRequestCount, retryQueues;      // on-demand mode: voxel -> table row, the request list, the vertices to shade again
    uint32_t voxRows = 0, voxRowsUsed = 0, nVoxels = 0;                   // rows the tables can hold / hold
    hprt::DevBuf rayStats, pixelStatsLocal, pixelStatsFilm; bool pixelStatsValid = false;   // HPRT_RENDER_PIXEL_STATS
    // render-time state
    hprt::DevBuf planes;                                    // backing store of the path streams (Workspace)
    hprt::DevBuf apiRays, apiHits;                          // stream copies of the plane-layout arguments of the *_device calls
    hprt::DevBuf queues, queueCounts;
    double aoKernelMs[3] = {0, 0, 0};                       // HIP-event time of k_ao_frame, k_ao_rays and k_ao_resolve in the last hprt_render_ao (hprt_debug_ao_kernel_seconds)
    hprt::DevBuf aoSlots, aoRays;                           // hprt_render_ao: the camera samples' streams and hit records; the hemisphere rays, terms and bytes
    // hprt_render_direct (device/direct.h): per camera sample the walk's state, stack, node rays, hits and hit records; per light sample
    // the item records and the two ray streams; the per-light tables.  dlKernelMs: HIP-event time of k_dl_shade, k_dl_rays, k_dl_resolve
    // and k_dl_advance in the last hprt_render_direct (hprt_debug_dl_kernel_seconds); dlSteps: tree-walk steps of its batches
    hprt::DevBuf dlSlots, dlRays, dlTables;
    double dlKernelMs[4] = {0, 0, 0, 0};
    uint64_t dlSteps = 0;
    // what CheckDirectScene refuses without touching the device: a material with an image texture; a material with a specular lobe that
    // SpecularReflect / SpecularTransmit can follow (mirror, smooth glass, uber with Kr, Kt or an opacity that is textured or not 1)
    bool hasImageTexture = false, hasSpecularLobe = false;
    hprt::DevBuf pixelXY, pixelOffset, Lall, film, irregular, irregularCount;
    hprt::DevBuf exOwnBegin, exOwnSrc, exOwnSample, exOwnPre, exFDest, exFDestBegin, exFGroupBegin, exFSrc, exFSample;
    // HPRT_RENDER_EXPORT_FOREIGN: the cross-tile film contributions of the last render, one record per (destination
    // pixel, source tile), sorted by both; applied by hprt_film_gather on the root in the single-GPU order
    hprt::DevBuf foreignRecords, exGroupDest, exGroupTile; uint32_t nForeignRecords = 0; bool foreignExported = false;
    int filmW = 0, filmH = 0;
    float *lastFilm = nullptr;                        // the device buffer the last hprt_render wrote: the caller's, or `film`
    uint32_t *hostCounts = nullptr;                   // pinned
    size_t filmPixels = 0;
    uint32_t nPrims = 0;
    // The walk every trace of the scene takes (Trace, capi_device.hip): the BVH walks until an hprt_scene_attach_* call attaches a
    // tree (AttachTree), whose walk then replaces them; attaching a tree replaces the one before.  treeNodes / treePrims back the
    // attached tree's descriptor: `kd` for the kd walk, `rbsp` for the RBSP and rbspkd walks, `bsppaper` (with its per-node axes in
    // treeAxes) for the general BSP walk and the kd-aware one (bsppaperkd).  kdShare: the rbspkd and bsppaperkd walks' kd
    // counter pair (DevRbspKd / DevBspPaperKd::kdCounters); pixelKdLocal / pixelKdFilm: their per-pixel kd share of HPRT_RENDER_PIXEL_STATS.
    // topOrder keeps the top-level prim_order (ordered -> creation number) to map a tree's creation-order primitives; instanced:
    // no tree walk
    enum class Walk { Bvh, Kd, Rbsp, RbspKd, BspPaper, BspPaperKd, KdInst, RbspInst, RbspKdInst, BspPaperInst, BspPaperKdInst } walk = Walk::Bvh;
    hprt::DevBuf treeNodes, treePrims, treeAxes; hprt::DevKd kd{}; hprt::DevRbsp rbsp{}; hprt::DevBspPaper bsppaper{};
    hprt::DevBuf kdShare, pixelKdLocal, pixelKdFilm; bool pixelKdValid = false;
    std::vector<uint32_t> topOrder; bool instanced = false;
    bool hasSubstrateBin = false;                     // some triangle carries BIN_SUBSTRATE: the substrate shading variant is launched
    // Two-level trees, the tree walks of an instanced scene (AttachTwoLevel, capi_device.hip): treeNodes / treePrims hold the nodes and
    // primitiveIndices of the top-level tree followed by every object tree's, instEntries one DevInstEntry per instance
    // (device/two_level.h).  kdinst: two-level kd-trees (hprt_scene_attach_kdinst, Walk::KdInst); rbspinst: two-level RBSP trees
    // (hprt_scene_attach_rbspinst; Walk::RbspInst, or Walk::RbspKdInst for kd-aware trees, which count their kd share in kdShare as
    // the rbspkd walk does); bsppaperinst: two-level general BSP trees (hprt_scene_attach_bsppaperinst; Walk::BspPaperInst, or
    // Walk::BspPaperKdInst for kd-aware trees with their kd share in kdShare), whose per-node axes — one per node of treeNodes — sit
    // in treeAxes.  objectOrder / objectPrimBase map an object tree's creation-order primitives as topOrder maps the top
    // level's; instanceObject: each instance's object definition
    hprt::DevBuf instEntries; hprt::DevKdInst kdinst{}; hprt::DevRbspInst rbspinst{}; hprt::DevBspPaperInst bsppaperinst{};
    std::vector<std::vector<uint32_t>> objectOrder; std::vector<uint32_t> objectPrimBase; std::vector<int32_t> instanceObject;
    ~HprtScene() { if (hostCounts) (void)hipHostFree(hostCounts); if (lastUse) (void)hipEventDestroy(lastUse); }
};

inline hprt::SceneCall::SceneCall(HprtScene *scene, hipStream_t stream) : lk(scene->mu), s(scene), st(stream) {
    if (s->lastUsePending && s->lastUse) (void)hipStreamWaitEvent(st, s->lastUse, 0);
}
inline void hprt::SceneCall::leave_async() {
    if (!s->lastUse && hipEventCreateWithFlags(&s->lastUse, hipEventDisableTiming) != hipSuccess) { s->lastUse = nullptr; (void)hipStreamSynchronize(st); s->lastUsePending = false; return; }
    s->lastUsePending = hipEventRecord(s->lastUse, st) == hipSuccess;
    if (!s->lastUsePending) (void)hipStreamSynchronize(st);
}
