// hprt — host half of the C ABI (include/hprt.h): scene front-end, baked scenes,
// BVH build, model -> scene description, Halton tables, film resolve, PFM writer.
// No HIP calls here; the device half lives in capi_device.hip.
#include <algorithm>
#include <new>
#include <stdexcept>
#include <cmath>
#include <limits>
#include <vector>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <type_traits>
#include "../../include/hprt.h"
#include "bsp_cost_device.h"
#include "bspnode_cost_device.h"
#include "bspnode_builder.h"
#include "bvh_builder.h"
#include "halton_tables.h"
#include "hlbvh_build_device.h"
#include "hprt_internal.h"
#include "kdop_cost_device.h"
#include "scene_model.h"
#include "hprt_math.h"
#include "wide_bvh.h"
#include "shadow_grid.h"
#include "distant_grid.h"

using namespace hprt;

namespace hprt {
thread_local std::string g_lastError;
int SetError(int code, const std::string &msg) { g_lastError = msg; return code; }
// No exception crosses the C ABI: every exported function that can allocate or parse is a function-try-block that ends here.
int HandleException() {
    try { throw; }
    catch (const std::bad_alloc &) { return SetError(HPRT_E_INVALID, "out of memory (or a size in the input that cannot be real)"); }
    catch (const std::length_error &e) { return SetError(HPRT_E_INVALID, std::string("a size in the input cannot be real: ") + e.what()); }
    catch (const std::exception &e) { return SetError(HPRT_E_INVALID, std::string("unexpected exception: ") + e.what()); }
    catch (...) { return SetError(HPRT_E_INVALID, "unexpected exception"); }
}
}  // namespace hprt

namespace {

// ---- the RBSP handles' builds, info and copies (hprt_rbsp_* and hprt_rbspkd_* below) ----
// The builder's view of a model's top-level primitives: world bounds, and the three world-space vertices of each triangle
// (Triangle::getBounds projects those; every other shape projects its world bound's corners)
void RbspModelPrims(const HprtModel *m, std::vector<float> *lo, std::vector<float> *hi, std::vector<float> *tri9, std::vector<uint8_t> *isTri) {
    ComputePrimBounds(m->sc, {}, lo, hi);
    const size_t n = lo->size() / 3;
    tri9->assign(9 * n, 0.f);
    isTri->assign(n, 0);
    size_t k = 0;
    for (const TopItem &ti : m->sc.top) {
        const ShapeDesc &sh = m->sc.shapes[ti.index];
        if (sh.kind != kTriangleMesh) { ++k; continue; }
        const MeshData &md = sh.mesh;
        for (uint32_t tr = 0; tr < md.nTris(); ++tr, ++k) {
            for (int v = 0; v < 3; ++v) memcpy(&(*tri9)[9 * k + 3 * v], &md.P[3 * (size_t)md.indices[3 * tr + v]], 12);
            (*isTri)[k] = 1;
        }
    }
}
// WorldBound of a triangle: Union(Bounds3f(p0, p1), p2) (shapes/triangle.cpp:180-186)
void RbspTriangleBounds(size_t n, const float *p9, std::vector<float> *lo, std::vector<float> *hi) {
    lo->resize(3 * n); hi->resize(3 * n);
    for (size_t i = 0; i < n; ++i)
        for (int d = 0; d < 3; ++d) {
            const float a = p9[9 * i + d], b = p9[9 * i + 3 + d], c = p9[9 * i + 6 + d];
            const float l = std::min(a, b), h = std::max(a, b);
            (*lo)[3 * i + d] = std::min(l, c); (*hi)[3 * i + d] = std::max(h, c);
        }
}
// ---- what the RBSP, general BSP and node-based BSP builds share: the costing hook's two users and the end of a build ----
// What a build does besides the host build (NULL: nothing).  device: the device-assisted build (hprt_*_build*_device) — nodes of
// at least min_candidates candidates are costed by the family's kernel (k_kdopcost, k_bspcost, k_sweepcost).  sink: the diagnostics
// hooks hprt_debug_*_root_* — the first maxNodes costed nodes are handed to the sink with the costs (and counts) the builder's own
// code gave them.
template <typename Opts, typename Sink>
struct BuildHook {
    bool device = false;
    const Opts *opts = nullptr;
    HprtBuildDeviceStats *stats = nullptr;
    Sink sink = nullptr; void *user = nullptr; uint32_t maxNodes = 0;
};
// Below this many candidates a node of a device-assisted build stays on the host: a launch and two copies cost more than the
// candidates do
constexpr uint32_t kDeviceMinCandidates = 1024;
// What the hook's callbacks keep for the end of the build
struct HookState { BuildDeviceStats bs; int rc = HPRT_OK; uint32_t seen = 0; };
// Installs hook into a builder's params (cost_hook.h).  open(): opens the family's device, HPRT_OK or a code with the error set.
// cost(rq, err): costs a node on it — 0, 1 (declined) or -1 with st->rc and *err.  emit(node, rq): hands a costed node to the sink.
template <typename Request, typename Hook, typename Open, typename Cost, typename Emit>
int InstallHook(const Hook *hook, CostHook<Request> *p, HookState *st, Open open, Cost cost, Emit emit) {
    if (hook && hook->device) {
        if (hook->stats) *hook->stats = HprtBuildDeviceStats{0, 0, 0, 0, 0.0};
        if (const int rc = open()) return rc;
        p->costMinCandidates = hook->opts && hook->opts->min_candidates ? hook->opts->min_candidates : kDeviceMinCandidates;
        p->stats = &st->bs;
        p->costFn = cost;
    } else if (hook && hook->sink) {
        p->costMinCandidates = 1;
        p->costFn = [=](const Request &rq, std::string *) -> int {
            if (st->seen >= hook->maxNodes) return 1;
            memset(rq.overflow, 1, rq.n);          // every candidate "flagged": the builder costs them all with its own code
            return 0;
        };
        p->costDone = [=](const Request &rq) { emit(st->seen++, rq); };
    }
    return HPRT_OK;
}
// "<what> of depth <depth> is deeper than the device walk's todo list", with the limit and the remedy when todoMax is given
std::string TooDeepMessage(const std::string &what, uint32_t depth, uint32_t todoMax = 0) {
    std::string msg = what + " of depth " + std::to_string(depth) + " is deeper than the device walk's todo list";
    if (todoMax) msg += " (" + std::to_string(todoMax) + " entries); lower \"maxdepth\"";
    return msg;
}
// The end of a build: the statistics out, the hook's failure or the builder's, and no tree deeper than the walk's todo list
template <typename Hook, typename Handle>
int FinishBuild(const Hook *hook, const HookState &st, const std::string &err, const char *what, uint32_t todoMax, std::unique_ptr<Handle> &t, Handle **out) {
    if (hook && hook->stats)
        *hook->stats = HprtBuildDeviceStats{st.bs.nodesDevice, st.bs.candidatesDevice, st.bs.candidatesRecosted, st.bs.nodesHost, st.bs.secondsDevice};
    if (st.rc != HPRT_OK) return SetError(st.rc, err);
    if (!err.empty()) return SetError(HPRT_E_UNSUPPORTED, err);
    if (t->tree.depth > todoMax) return SetError(HPRT_E_UNSUPPORTED, TooDeepMessage(what, t->tree.depth, todoMax));
    *out = t.release();
    return HPRT_OK;
}
// A family's device for the length of a build or a call
template <typename Device, void (*Destroy)(Device *)>
using DevicePtr = std::unique_ptr<Device, std::integral_constant<void (*)(Device *), Destroy>>;
using KdopDevicePtr = DevicePtr<KdopCostDevice, KdopCostDeviceDestroy>;
using BspDevicePtr = DevicePtr<BspCostDevice, BspCostDeviceDestroy>;
using BspNodeDevicePtr = DevicePtr<BspNodeCostDevice, BspNodeCostDeviceDestroy>;

// ---- the RBSP handles' builds (Handle HprtRbsp with Params HprtRbspParams, or HprtRbspKd, the kd-aware cost model, with
// HprtRbspKdParams; params NULL keeps p) ----
typedef void (*RbspNodeSink)(void *user, uint32_t node, const void *edges, uint32_t n_edges, const void *scalars, const void *cands, size_t n,
                             const float *costs, const float *costs_fixed);
using RbspHook = BuildHook<HprtBuildDeviceOpts, RbspNodeSink>;

// HprtRbspParams / HprtRbspKdParams over the Accelerator line's (or the defaults'); params NULL keeps *p
template <typename Params>
void ApplyRbspParams(const Params *params, RbspParams *p) {
    if (!params) return;
    p->isectCost = params->isect_cost; p->travCost = params->trav_cost; p->emptyBonus = params->empty_bonus;
    p->maxPrims = params->max_prims; p->maxDepth = params->max_depth; p->nDirections = params->n_directions; p->threads = params->threads;
    if constexpr (std::is_same<Params, HprtRbspKdParams>::value) p->kdTravCost = params->kd_trav_cost;
}
template <typename Handle, typename Params>
int BuildRbsp(size_t n, const float *lo, const float *hi, const float *tri9, const uint8_t *isTri, const Params *params, RbspParams p,
                     Handle **out, const RbspHook *hook = nullptr) {
    constexpr bool kdAware = std::is_same<Handle, HprtRbspKd>::value;
    p.kdAware = kdAware;
    *out = nullptr;
    ApplyRbspParams(params, &p);
    if (p.nDirections != 3 && p.nDirections != 7 && p.nDirections != 9 && p.nDirections != 13)
        return SetError(HPRT_E_UNSUPPORTED, "nbDirections " + std::to_string(p.nDirections) + " is not supported (3, 7, 9 or 13)");
    std::unique_ptr<Handle> t(new Handle());
    KdopDevicePtr dev;                                   // freed when the build ends or fails
    HookState st;
    const int rc = InstallHook<RbspCostRequest>(hook, &p, &st, [&]() -> int {
        std::string derr;
        KdopCostDevice *d = nullptr;
        const int rc = KdopCostDeviceCreate(hook->opts ? hook->opts->device : 0, hook->opts ? hook->opts->max_edges : 0u, &d, &derr);
        dev.reset(d);
        return rc != HPRT_OK ? SetError(rc, derr) : HPRT_OK;
    }, [&](const RbspCostRequest &rq, std::string *e) -> int {
        if (rq.nEdges > KdopCostDeviceCapacity(dev.get())) return 1;      // the whole node on the host
        st.rc = KdopCostDeviceRun(dev.get(), rq.mesh, rq.nEdges, rq.dirs, rq.M, rq.kdAware, rq.sc, rq.cands, rq.n, rq.costs, rq.costsFixed, rq.overflow, e);
        return st.rc == HPRT_OK ? 0 : -1;
    }, [=](uint32_t node, const RbspCostRequest &rq) {
        hook->sink(hook->user, node, rq.mesh, rq.nEdges, &rq.sc, rq.cands, rq.n, rq.costs, rq.costsFixed);
    });
    if (rc != HPRT_OK) return rc;
    const std::string err = BuildRbspTree(n, lo, hi, tri9, isTri, p, &t->tree);
    return FinishBuild(hook, st, err, "RBSP tree", RBSP_TODO_MAX, t, out);
}
// hprt_rbsp_build / hprt_rbspkd_build: the model's primitives and its Accelerator line (dflt); `what` names the tree in messages
template <typename Handle, typename Params>
int BuildRbspFromModel(const char *fn, const char *what, const HprtModel *m, const Params *params, const RbspParams &dflt, Handle **out,
                       const RbspHook *hook = nullptr) {
    if (out) *out = nullptr;
    if (!m || !out) return SetError(HPRT_E_INVALID, std::string(fn) + ": null argument");
    if (m->sc.nObjects != 0 || !m->sc.instances.empty())
        return SetError(HPRT_E_UNSUPPORTED, std::string(what) + " trees over object instances are not supported (the scene keeps its BVH)");
    std::vector<float> lo, hi, tri9;
    std::vector<uint8_t> isTri;
    RbspModelPrims(m, &lo, &hi, &tri9, &isTri);
    return BuildRbsp(lo.size() / 3, lo.data(), hi.data(), tri9.data(), isTri.data(), params, dflt, out, hook);
}
template <typename Handle, typename Params>
int BuildRbspFromTriangles(const char *fn, size_t n, const float *p9, const Params *params, Handle **out, const RbspHook *hook = nullptr) {
    if (out) *out = nullptr;
    if (!out || (n && !p9)) return SetError(HPRT_E_INVALID, std::string(fn) + ": null argument");
    if (n > 0x3fffffffull) return SetError(HPRT_E_UNSUPPORTED, "more than 2^30 primitives");
    std::vector<float> lo, hi;
    RbspTriangleBounds(n, p9, &lo, &hi);
    std::vector<uint8_t> isTri(n, 1);
    return BuildRbsp(n, lo.data(), hi.data(), p9, isTri.data(), params, RbspParams(), out, hook);
}
// info[0..4] of either handle; info[5..6] (kd / oblique interior nodes) only for an rbspkd tree
int RbspInfo(const char *fn, const RbspTree *t, uint32_t *info, bool kdSplit) {
    if (!t || !info) return SetError(HPRT_E_INVALID, std::string(fn) + ": null argument");
    info[0] = (uint32_t)t->nodes.size(); info[1] = t->leaves; info[2] = (uint32_t)t->primIndices.size();
    info[3] = t->depth; info[4] = t->M;
    if (kdSplit) RbspInteriorCounts(*t, &info[5], &info[6]);
    return HPRT_OK;
}
int RbspCopy(const char *fn, const RbspTree *t, void *nodes8, uint32_t *primIndices, float *directions) {
    if (!t) return SetError(HPRT_E_INVALID, std::string(fn) + ": null argument");
    if (nodes8) memcpy(nodes8, t->nodes.data(), t->nodes.size() * sizeof(RbspNode));
    if (primIndices && !t->primIndices.empty()) memcpy(primIndices, t->primIndices.data(), t->primIndices.size() * 4);
    if (directions) memcpy(directions, t->directions.data(), t->directions.size() * 4);
    return HPRT_OK;
}

// ---- two-level RBSP trees (BuildRbspInst below; pbrtObjectInstance, core/api.cpp:1794-1819, under Accelerator "rbsp" / "rbspkd") ----
// tri9 / isTri as BuildRbspTree takes them, for the n primitives of the top level (object < 0; an instance is no triangle: its
// projections are those of its world bound's corners, Primitive::getBounds, core/primitive.h:72-80) or of one object, in the order
// of ComputePrimBounds / ComputeObjectPrimBounds
void RbspPrimTriangles(const SceneModel &sc, int object, size_t n, std::vector<float> *tri9, std::vector<uint8_t> *isTri) {
    tri9->assign(9 * n, 0.f);
    isTri->assign(n, 0);
    size_t k = 0;
    auto shape = [&](const ShapeDesc &sh) {
        if (sh.kind != kTriangleMesh) { ++k; return; }
        const MeshData &md = sh.mesh;
        for (uint32_t tr = 0; tr < md.nTris(); ++tr, ++k) {
            for (int v = 0; v < 3; ++v) memcpy(&(*tri9)[9 * k + 3 * v], &md.P[3 * (size_t)md.indices[3 * tr + v]], 12);
            (*isTri)[k] = 1;
        }
    };
    if (object < 0) {
        for (const TopItem &ti : sc.top) { if (ti.kind == 0) shape(sc.shapes[ti.index]); else ++k; }
    } else {
        for (const ShapeDesc &sh : sc.shapes) if (sh.object == object) shape(sh);
    }
}

// ---- the general BSP handles' builds and copies (hprt_bsppaper_* and hprt_bsppaperkd_* below) ----
// Handle HprtBspPaper with Params HprtBspPaperParams, or HprtBspPaperKd (the kd-aware cost model and node flags) with
// HprtBspPaperKdParams; params NULL keeps p
// What the diagnostics hook hprt_debug_bsp_root_nodes hands out (BuildHook's sink)
struct HprtDebugBspNode {
    const void *edges; uint32_t n_edges;              // 32-byte records (v1, v2, f1, f2), face ids below 2 M
    const float *dirs; uint32_t M;                    // the node's direction list
    const void *scalars;                              // bspcost::Scalars (10 words)
    const void *cands; size_t n, n_axis;              // 32-byte records (k, i, nBelow, nAbove, t, axis); axis candidates first
    const void *bvh_nodes; uint32_t n_bvh;            // 32-byte LinearBVHNode records of the BVH over the node's primitives
    const uint32_t *prim_order, *prim_nums; uint32_t n_prims;
    const float *bmin, *bmax, *tri9; const uint8_t *is_tri; size_t n_total;      // the build's primitives
    const float *costs, *costs_fixed;                 // the builder's own (costs_fixed NULL unless kd-aware); NULL as an input
    uint32_t level;                                   // the node's depth below the root
};
typedef void (*BspNodeSink)(void *user, uint32_t node, const HprtDebugBspNode *nd);
using BspHook = BuildHook<HprtBspBuildDeviceOpts, BspNodeSink>;
constexpr uint32_t BspPaperTodoMax(bool kdAware) { return kdAware ? (uint32_t)BSPPAPERKD_TODO_MAX : (uint32_t)BSPPAPER_TODO_MAX; }
// The node of a request as bsp_cost.h reads it: compact face ids and the directions that own a face.  False: the node's own
// mesh, direction list or faces exceed the capacities (it is declined whole), or a face id is not below 2 M.
struct BspCompact { std::vector<bspcost::Edge> mesh; std::vector<uint32_t> cdir; uint32_t nD = 0; };
bool BspCompactRequest(const BspCostRequest &rq, const uint32_t cap[4], BspCompact *c) {
    if (rq.nEdges > cap[0] || rq.M == 0 || rq.M > BSP_MAX_DIRS) return false;
    for (uint32_t k = 0; k < rq.nEdges; ++k)
        if (rq.mesh[k].f1 >= 2 * rq.M || rq.mesh[k].f2 >= 2 * rq.M) return false;
    c->mesh.resize(rq.nEdges); c->cdir.resize(rq.M);
    bspcost::CompactNode(rq.mesh, rq.nEdges, rq.M, c->mesh.data(), c->cdir.data(), &c->nD);
    return 2 * c->nD <= cap[1];
}
// Takes over what a costing wrote beside rq's own arrays: the fixed costs and the counts of the candidates it has costed
void BspTakeResults(const BspCostRequest &rq, const float *fixed, const uint32_t *counts) {
    for (size_t k = 0; k < rq.n; ++k) {
        if (rq.overflow[k]) continue;
        if (rq.costsFixed) rq.costsFixed[k] = fixed[k];
        rq.cands[k].nBelow = counts[2 * k]; rq.cands[k].nAbove = counts[2 * k + 1];
    }
}
// bsp_cost.h on the host, one candidate after the other (the diagnostics hook's impl 1).  1: the node is declined.
int BspCostRestated(const BspCostRequest &rq) {
    uint32_t cap[4];
    if (!bspcost::Capacities(rq.sc, cap)) return -1;
    BspCompact cn;
    if (!BspCompactRequest(rq, cap, &cn)) return 1;
    using namespace bspcost;
    std::vector<Q> words(kStoreWords);
    uint8_t list[BSP_MAX_FACE_EDGES];
    uint32_t stack[BSP_MAX_STACK];
    Store st;
    st.left = words.data(); st.right = words.data() + 2 * BSP_MAX_EDGES; st.fv = words.data() + 4 * BSP_MAX_EDGES; st.stride = 1;
    st.flist = list; st.fstride = 1; st.stack = stack; st.sstride = 1;
    st.capEdges = cap[0]; st.capFaces = cap[1]; st.capFaceEdges = cap[2]; st.capStack = cap[3];
    const Node nd{cn.mesh.data(), rq.nEdges, rq.dirs, rq.M, cn.cdir.data(), cn.nD, rq.bvh, rq.nBvh, rq.primOrder, rq.primNums, rq.nPrims,
                  rq.bmin, rq.bmax, rq.tri9, rq.isTri, (uint32_t)rq.nTotal};
    std::vector<float> fixed(rq.n);
    std::vector<uint32_t> counts(2 * rq.n);
    for (size_t k = 0; k < rq.n; ++k)
        CostCandidate(nd, rq.kdAware, rq.sc, rq.cands[k], st, &rq.costs[k], &fixed[k], &counts[2 * k], &counts[2 * k + 1], &rq.overflow[k]);
    BspTakeResults(rq, fixed.data(), counts.data());
    return 0;
}
// k_bspcost over a request (the device-assisted build, and the diagnostics hook's impl 2).  0, 1 (declined) or -1 with *rc / *err.
int BspCostOnDevice(BspCostDevice *dev, const uint32_t cap[4], const BspCostRequest &rq, int *rc, std::string *err) {
    BspCompact cn;
    if (!BspCompactRequest(rq, cap, &cn)) return 1;
    std::vector<float> fixed(rq.n);
    std::vector<uint32_t> counts(2 * rq.n);
    *rc = BspCostDeviceRun(dev, cn.mesh.data(), rq.nEdges, rq.dirs, rq.M, cn.cdir.data(), cn.nD, rq.kdAware, rq.sc, rq.cands, rq.n, rq.nAxis, rq.bvh, rq.nBvh,
                           rq.primOrder, rq.primNums, rq.nPrims, rq.costs, fixed.data(), counts.data(), rq.overflow, err);
    if (*rc != HPRT_OK) return -1;
    BspTakeResults(rq, fixed.data(), counts.data());
    return 0;
}

template <typename Handle, typename Params>
int BuildBspPaper(size_t n, const float *lo, const float *hi, const float *tri9, const uint8_t *isTri, const Params *params,
                  BspPaperParams p, Handle **out, const BspHook *hook = nullptr) {
    constexpr bool kdAware = std::is_same<Handle, HprtBspPaperKd>::value;
    p.kdAware = kdAware;
    if (hook) *out = nullptr;
    if (params) {
        p.isectCost = params->isect_cost; p.travCost = params->trav_cost; p.emptyBonus = params->empty_bonus;
        p.maxPrims = params->max_prims; p.maxDepth = params->max_depth; p.threads = params->threads;
        if constexpr (kdAware) p.kdTravCost = params->kd_trav_cost;
    }
    std::unique_ptr<Handle> t(new Handle());
    BspDevicePtr dev;                                    // freed when the build ends or fails
    HookState st;
    uint32_t cap[4] = {0, 0, 0, 0};
    const int rc = InstallHook<BspCostRequest>(hook, &p, &st, [&]() -> int {
        const HprtBspBuildDeviceOpts *o = hook->opts;
        const uint32_t asked[4] = {o ? o->max_edges : 0u, o ? o->max_faces : 0u, o ? o->max_face_edges : 0u, o ? o->max_stack : 0u};
        std::string derr;
        BspCostDevice *d = nullptr;
        const int rc = BspCostDeviceCreate(o ? o->device : 0, asked, n, lo, hi, tri9, isTri, &d, &derr);
        dev.reset(d);
        if (rc != HPRT_OK) return SetError(rc, derr);
        bspcost::Scalars sc{};
        sc.maxEdges = asked[0]; sc.maxFaces = asked[1]; sc.maxFaceEdges = asked[2]; sc.maxStack = asked[3];
        bspcost::Capacities(sc, cap);
        return HPRT_OK;
    }, [&](const BspCostRequest &rq, std::string *e) -> int { return BspCostOnDevice(dev.get(), cap, rq, &st.rc, e); },
    [=](uint32_t node, const BspCostRequest &rq) {
        const HprtDebugBspNode nd{rq.mesh, rq.nEdges, rq.dirs, rq.M, &rq.sc, rq.cands, rq.n, rq.nAxis, rq.bvhNodes, rq.nBvh, rq.primOrder, rq.primNums,
                                  rq.nPrims, rq.bmin, rq.bmax, rq.tri9, rq.isTri, rq.nTotal, rq.costs, rq.costsFixed, rq.level};
        hook->sink(hook->user, node, &nd);
    });
    if (rc != HPRT_OK) return rc;
    const std::string err = BuildBspPaperTree(n, lo, hi, tri9, isTri, p, &t->tree);
    return FinishBuild(hook, st, err, kdAware ? "bsppaperkd tree" : "bsppaper tree", BspPaperTodoMax(kdAware), t, out);
}
// nodes20: the reference's 5 words per node (BSPNode / BSPKdNode)
int BspPaperCopy(const BspPaperTree &b, void *nodes20, uint32_t *primIndices) {
    if (nodes20)
        for (size_t k = 0; k < b.nodes.size(); ++k) {
            uint32_t w[5] = {b.nodes[k].a, b.nodes[k].b, 0, 0, 0};
            memcpy(&w[2], &b.axes[3 * k], 12);
            memcpy((char *)nodes20 + 20 * k, w, 20);
        }
    if (primIndices && !b.primIndices.empty()) memcpy(primIndices, b.primIndices.data(), b.primIndices.size() * 4);
    return HPRT_OK;
}

// ---- the node-based BSP trees' builds (hprt_bspnode_* and hprt_bspnodekd_* below): Handle HprtBspPaper for the plain and withkd
// forms, HprtBspPaperKd for the fastkd form; params NULL keeps p (the scene's Accelerator line)
// What the diagnostics hook hprt_debug_bspnode_root_nodes hands out (BuildHook's sink)
struct HprtDebugBspSweepNode {
    const void *edges; uint32_t n_edges;              // 32-byte records (v1, v2, f1, f2), face ids below 2 M
    const float *dirs; uint32_t M;                    // the node's own direction list
    const void *sweep; uint32_t n_dirs;               // 16-byte records (axis, kind): the directions the node sweeps
    const void *scalars;                              // bspcost::Scalars (10 words)
    const void *cands; size_t n;                      // 16-byte records (k, nBelow, nAbove, t) in (direction, edge) order
    const float *costs, *costs_fixed;                 // the builder's own (costs_fixed NULL unless fastkd); NULL as an input
    uint32_t level;                                   // the node's depth below the root
};
typedef void (*BspSweepNodeSink)(void *user, uint32_t node, const HprtDebugBspSweepNode *nd);
using BspNodeHook = BuildHook<HprtBspBuildDeviceOpts, BspSweepNodeSink>;
// The node of a request as bspnode_cost.h reads it.  False: the node's own mesh, direction list, faces or sweep exceed the
// capacities (it is declined whole), or a face id or a candidate's direction is out of range.
bool BspNodeCompactRequest(const BspNodeCostRequest &rq, const uint32_t cap[4], BspCompact *c) {
    if (rq.nEdges > cap[0] || rq.M == 0 || rq.M > BSP_MAX_DIRS || rq.nDirs == 0 || rq.nDirs > BSPNODE_MAX_SWEEP_DIRS) return false;
    for (uint32_t k = 0; k < rq.nEdges; ++k)
        if (rq.mesh[k].f1 >= 2 * rq.M || rq.mesh[k].f2 >= 2 * rq.M) return false;
    for (size_t k = 0; k < rq.n; ++k)
        if (rq.cands[k].k >= rq.nDirs) return false;
    c->mesh.resize(rq.nEdges); c->cdir.resize(rq.M);
    bspcost::CompactNode(rq.mesh, rq.nEdges, rq.M, c->mesh.data(), c->cdir.data(), &c->nD);
    return 2 * c->nD <= cap[1];
}
// bspnode_cost.h on the host (the diagnostics hook's impl 1), over storage sized exactly to the capacities in force.  1: declined.
int BspNodeCostRestated(const BspNodeCostRequest &rq) {
    uint32_t cap[4];
    if (!bspcost::Capacities(rq.sc, cap)) return -1;
    BspCompact cn;
    if (!BspNodeCompactRequest(rq, cap, &cn)) return 1;
    std::vector<bspcost::Q> words(4 * (size_t)cap[0] + 2 * (size_t)cap[1]);
    std::vector<uint8_t> list(cap[2]);
    bspnodecost::CostNode(cn.mesh.data(), rq.nEdges, rq.dirs, rq.M, cn.cdir.data(), cn.nD, rq.fastKd, rq.sc, rq.sweep, rq.nDirs, rq.cands, rq.n, cap,
                          words.data(), list.data(), rq.costs, rq.costsFixed, rq.overflow);
    return 0;
}
// k_sweepcost over a request (the device-assisted build, and the diagnostics hook's impl 2).  0, 1 (declined) or -1 with *rc / *err.
int BspNodeCostOnDevice(BspNodeCostDevice *dev, const uint32_t cap[4], const BspNodeCostRequest &rq, int *rc, std::string *err) {
    BspCompact cn;
    if (!BspNodeCompactRequest(rq, cap, &cn)) return 1;
    *rc = BspNodeCostDeviceRun(dev, cn.mesh.data(), rq.nEdges, rq.dirs, rq.M, cn.cdir.data(), cn.nD, rq.fastKd, rq.sc, rq.sweep, rq.nDirs, rq.cands, rq.n,
                               rq.costs, rq.costsFixed, rq.overflow, err);
    return *rc != HPRT_OK ? -1 : 0;
}

// HprtBspNodeParams over the Accelerator line's (or the defaults'); params NULL keeps *p
void ApplyBspNodeParams(const HprtBspNodeParams *params, BspNodeParams *p) {
    if (!params) return;
    p->chooser = params->chooser; p->form = params->form; p->nDirections = params->n_directions; p->seed = params->seed;
    p->isectCost = params->isect_cost; p->travCost = params->trav_cost; p->kdTravCost = params->kd_trav_cost; p->emptyBonus = params->empty_bonus;
    p->maxPrims = params->max_prims; p->maxDepth = params->max_depth; p->threads = params->threads;
}
// The costing hook of a node-based build and what it keeps until the build ends or fails: installed once into the params, it serves
// every BuildBspNodeTree call made with them — the one tree of hprt_bspnode_build_device, every tree of hprt_bspnodeinst_build_device
// — through one device session, and st.bs sums the statistics over those calls.  The params hold lambdas that point back here.
struct BspNodeHookState {
    BspNodeDevicePtr dev;
    HookState st;
    uint32_t cap[4] = {0, 0, 0, 0};
    BspNodeHookState() = default;
    BspNodeHookState(const BspNodeHookState &) = delete;
    int Install(const BspNodeHook *hook, BspNodeParams *p) {
        return InstallHook<BspNodeCostRequest>(hook, p, &st, [&]() -> int {
            // the refusals that do not depend on the primitives come first, as the host entry gives them, with or without a device
            const std::string refused = BspNodeRefuseParams(*p);
            if (!refused.empty()) return SetError(HPRT_E_UNSUPPORTED, refused);
            const HprtBspBuildDeviceOpts *o = hook->opts;
            const uint32_t asked[3] = {o ? o->max_edges : 0u, o ? o->max_faces : 0u, o ? o->max_face_edges : 0u};      // (max_stack: no BVH here)
            std::string derr;
            BspNodeCostDevice *d = nullptr;
            const int rc = BspNodeCostDeviceCreate(o ? o->device : 0, asked, &d, &derr);
            dev.reset(d);
            if (rc != HPRT_OK) return SetError(rc, derr);
            bspcost::Scalars sc{};
            sc.maxEdges = asked[0]; sc.maxFaces = asked[1]; sc.maxFaceEdges = asked[2];
            bspcost::Capacities(sc, cap);
            return HPRT_OK;
        }, [this](const BspNodeCostRequest &rq, std::string *e) -> int { return BspNodeCostOnDevice(dev.get(), cap, rq, &st.rc, e); },
        [=](uint32_t node, const BspNodeCostRequest &rq) {
            const HprtDebugBspSweepNode nd{rq.mesh, rq.nEdges, rq.dirs, rq.M, rq.sweep, rq.nDirs, &rq.sc, rq.cands, rq.n, rq.costs, rq.costsFixed, rq.level};
            hook->sink(hook->user, node, &nd);
        });
    }
};

template <typename Handle>
int BuildBspNode(const char *fn, size_t n, const float *lo, const float *hi, const float *tri9, const uint8_t *isTri, const HprtBspNodeParams *params,
                 BspNodeParams p, Handle **out, const BspNodeHook *hook = nullptr) {
    constexpr bool fastKd = std::is_same<Handle, HprtBspPaperKd>::value;
    if (hook) *out = nullptr;
    ApplyBspNodeParams(params, &p);
    if ((p.form == BSPNODE_FASTKD) != fastKd)
        return SetError(HPRT_E_INVALID, std::string(fn) + (fastKd ? ": takes the fastkd form only (the plain and withkd forms are hprt_bspnode_build's)"
                                                                  : ": takes the plain and withkd forms only (the fastkd form is hprt_bspnodekd_build's)"));
    std::unique_ptr<Handle> t(new Handle());
    BspNodeHookState hs;                                 // (the device is freed when the build ends or fails)
    if (const int rc = hs.Install(hook, &p)) return rc;
    const std::string err = BuildBspNodeTree(n, lo, hi, tri9, isTri, p, &t->tree);
    return FinishBuild(hook, hs.st, err, "node-based BSP tree", BspPaperTodoMax(fastKd), t, out);
}
template <typename Handle>
int BuildBspNodeFromModel(const char *fn, const HprtModel *m, const HprtBspNodeParams *params, Handle **out, const BspNodeHook *hook = nullptr) {
    if (!m || !out) return SetError(HPRT_E_INVALID, std::string(fn) + ": null argument");
    if (hook) *out = nullptr;
    if (m->sc.nObjects != 0 || !m->sc.instances.empty())
        return SetError(HPRT_E_UNSUPPORTED, "node-based BSP trees over object instances are not supported (the scene keeps its BVH)");
    BspNodeParams p = m->sc.opt.bspnode;
    if (!params && !BspNodeAccelerator(m->sc.opt.accelerator, &p.chooser, &p.form))
        return SetError(HPRT_E_INVALID, std::string(fn) + ": the scene's Accelerator \"" + m->sc.opt.accelerator + "\" is no node-based BSP tree; pass params");
    std::vector<float> lo, hi, tri9;
    std::vector<uint8_t> isTri;
    RbspModelPrims(m, &lo, &hi, &tri9, &isTri);
    return BuildBspNode(fn, lo.size() / 3, lo.data(), hi.data(), tri9.data(), isTri.data(), params, p, out, hook);
}
template <typename Handle>
int BuildBspNodeFromTriangles(const char *fn, size_t n, const float *p9, const HprtBspNodeParams *params, Handle **out, const BspNodeHook *hook = nullptr) {
    if (!out || !params || (n && !p9)) return SetError(HPRT_E_INVALID, std::string(fn) + ": null argument");
    if (hook) *out = nullptr;
    if (n > 0x0fffffffull) return SetError(HPRT_E_UNSUPPORTED, "more than 2^28 primitives");
    std::vector<float> lo, hi;
    RbspTriangleBounds(n, p9, &lo, &hi);
    std::vector<uint8_t> isTri(n, 1);
    return BuildBspNode(fn, n, lo.data(), hi.data(), p9, isTri.data(), params, BspNodeParams(), out, hook);
}

// ---- trees given as arrays (the hprt_debug_*_from_arrays hooks below): what a builder would have filled in, then the builder's own
// structural check and the walk's depth limit, so that the handle is an ordinary one ----
uint32_t CountLeaves(const std::vector<BspNode> &nodes, uint32_t mask, uint32_t leafTag) {
    return (uint32_t)std::count_if(nodes.begin(), nodes.end(), [&](const BspNode &nd) { return (nd.b & mask) == leafTag; });
}
template <typename Handle>
int RbspFromArrays(const char *fn, uint32_t M, size_t nNodes, const uint32_t *nodes8, size_t nIdx, const uint32_t *idx, uint32_t nPrims,
                   const float *bounds6, Handle **out) {
    if (!out || !nodes8 || !bounds6 || (nIdx && !idx)) return SetError(HPRT_E_INVALID, std::string(fn) + ": null argument");
    std::unique_ptr<Handle> t(new Handle());
    RbspTree &r = t->tree;
    if (!RbspDirections(M, &r.directions)) return SetError(HPRT_E_UNSUPPORTED, "nbDirections " + std::to_string(M) + " is not supported (3, 7, 9 or 13)");
    r.M = M; r.nPrims = nPrims;
    r.nodes.resize(nNodes);
    memcpy(r.nodes.data(), nodes8, nNodes * sizeof(RbspNode));
    r.primIndices.assign(idx, idx + nIdx);
    memcpy(r.bounds, bounds6, sizeof(r.bounds));
    const char *bad = CheckRbspTree(r, &r.depth);
    if (*bad) return SetError(HPRT_E_INVALID, std::string("malformed tree: ") + bad);
    r.maxDepth = r.depth; r.leaves = CountLeaves(r.nodes, RbspBitMask(M), M);
    if (r.depth > RBSP_TODO_MAX) return SetError(HPRT_E_UNSUPPORTED, TooDeepMessage("RBSP tree", r.depth, RBSP_TODO_MAX));
    *out = t.release();
    return HPRT_OK;
}
// axisNodes / planeNodes of a hand-made general BSP tree (one axis per node), which has no sweep: its axis nodes are the kd nodes, or
// those along a coordinate axis
void CountHandMadeInterior(BspPaperTree *b) {
    const uint32_t mask = b->kdAware ? (uint32_t)BSPPAPERKD_MASK : (uint32_t)BSPPAPER_MASK, leafTag = b->kdAware ? (uint32_t)BSPPAPERKD_LEAF : 1u;
    b->axisNodes = b->planeNodes = 0;
    for (size_t k = 0; k < b->nodes.size(); ++k) {
        const uint32_t kind = b->nodes[k].b & mask;
        if (kind == leafTag) continue;
        const float *a = &b->axes[3 * k];
        const bool axisNode = b->kdAware ? kind < BSPPAPERKD_LEAF : (a[0] != 0) + (a[1] != 0) + (a[2] != 0) == 1;
        ++(axisNode ? b->axisNodes : b->planeNodes);
    }
}
// nodes20: 5 words per node, as BspPaperCopy writes them
template <typename Handle>
int BspPaperFromArrays(const char *fn, size_t nNodes, const uint32_t *nodes20, size_t nIdx, const uint32_t *idx, uint32_t nPrims, const float *bounds6,
                       Handle **out) {
    constexpr bool kdAware = std::is_same<Handle, HprtBspPaperKd>::value;
    if (!out || !nodes20 || !bounds6 || (nIdx && !idx)) return SetError(HPRT_E_INVALID, std::string(fn) + ": null argument");
    std::unique_ptr<Handle> t(new Handle());
    BspPaperTree &b = t->tree;
    b.kdAware = kdAware; b.nPrims = nPrims;
    b.nodes.resize(nNodes); b.axes.resize(3 * nNodes);
    for (size_t k = 0; k < nNodes; ++k) {
        b.nodes[k] = BspNode{nodes20[5 * k], nodes20[5 * k + 1]};
        memcpy(&b.axes[3 * k], &nodes20[5 * k + 2], 12);
    }
    b.primIndices.assign(idx, idx + nIdx);
    memcpy(b.bounds, bounds6, sizeof(b.bounds));
    const char *bad = kdAware ? CheckBspPaperKdTree(b, &b.depth) : CheckBspPaperTree(b, &b.depth);
    if (*bad) return SetError(HPRT_E_INVALID, std::string("malformed tree: ") + bad);
    b.maxDepth = b.depth;
    b.leaves = kdAware ? CountLeaves(b.nodes, BSPPAPERKD_MASK, BSPPAPERKD_LEAF) : CountLeaves(b.nodes, BSPPAPER_MASK, 1u);
    CountHandMadeInterior(&b);
    if (b.depth > BspPaperTodoMax(kdAware))
        return SetError(HPRT_E_UNSUPPORTED, TooDeepMessage(kdAware ? "bsppaperkd tree" : "bsppaper tree", b.depth, BspPaperTodoMax(kdAware)));
    *out = t.release();
    return HPRT_OK;
}

// ---- two-level trees (hprt_kdinst_*, hprt_rbspinst_* and hprt_bsppaperinst_* below; pbrtObjectInstance, core/api.cpp:1794-1819):
// Handle is HprtKdInst, HprtRbspInst or HprtBspPaperInst (HprtTwoLevel, hprt_internal.h), Tree its KdTree, RbspTree or BspPaperTree ----
// The walk keeps the top-level tree's todo entries, one saved top-level position and the object tree's entries in one list of
// todoMax entries (device/kdinst_walk.hip, device/bspinst_walk.h); what: the tree's name in the message
template <typename Tree>
int CheckTwoLevelDepth(const HprtTwoLevel<Tree> &t, const char *what, uint32_t todoMax) {
    uint32_t deepest = 0;
    for (const Tree &o : t.objects) if (!o.nodes.empty()) deepest = std::max(deepest, o.depth);
    if ((uint64_t)t.top.depth + deepest + 1u > todoMax)
        return SetError(HPRT_E_UNSUPPORTED, std::string("two-level ") + what + ": top-level depth " + std::to_string(t.top.depth) + " + deepest object depth " +
                                            std::to_string(deepest) + " + 1 is more than the device walk's todo list holds (" + std::to_string(todoMax) +
                                            " entries); lower \"maxdepth\"");
    return HPRT_OK;
}
int CheckTwoLevelDepth(const HprtKdInst &t) { return CheckTwoLevelDepth(t, "kd-tree", KD_TODO_MAX); }
int CheckTwoLevelDepth(const HprtRbspInst &t) { return CheckTwoLevelDepth(t, "RBSP tree", RBSP_TODO_MAX); }
int CheckTwoLevelDepth(const HprtBspPaperInst &t) {
    return t.kdAware ? CheckTwoLevelDepth(t, "bsppaperkd tree", BSPPAPERKD_TODO_MAX) : CheckTwoLevelDepth(t, "bsppaper tree", BSPPAPER_TODO_MAX);
}
// The build of either handle: one tree per object of more than one primitive, over the object's primitives in object space, and the
// top-level tree over the top-level items, an instance bounded by TransformedPrimitive::WorldBound.  buildTree(object, n, lo, hi,
// &tree): the tree over the n primitives of one object or (object < 0) of the top level, returning what went wrong ("": nothing);
// bareObject(n, lo, hi, &tree): what the handle holds of an object of n < 2 primitives, which gets no tree.
template <typename Handle, typename BuildTree, typename BareObject>
int BuildTwoLevel(const SceneModel &sc, std::unique_ptr<Handle> t, BuildTree buildTree, BareObject bareObject, Handle **out) {
    for (const InstanceDesc &in : sc.instances) t->instanceObject.push_back(in.object);
    t->objects.resize(sc.nObjects);
    // TransformedPrimitive::WorldBound needs the wrapped primitive's bounds: the object accelerator's (the union of its primitives'
    // bounds), or the lone primitive's own — one-node trees that hold them, which is all ComputePrimBounds reads (bvh_builder.h)
    std::vector<BvhTree> objectBounds(sc.nObjects);
    std::vector<float> lo, hi;
    for (uint32_t o = 0; o < sc.nObjects; ++o) {
        ComputeObjectPrimBounds(sc, (int)o, &lo, &hi);
        const size_t n = lo.size() / 3;
        if (n > 0x3fffffffull) return SetError(HPRT_E_UNSUPPORTED, "more than 2^30 primitives");
        if (n > 1) {      // (core/api.cpp:1798: only more than one primitive gets an accelerator)
            const std::string err = buildTree((int)o, n, lo.data(), hi.data(), &t->objects[o]);
            if (!err.empty()) return SetError(HPRT_E_UNSUPPORTED, "object " + std::to_string(o) + ": " + err);
        } else bareObject(n, lo.data(), hi.data(), &t->objects[o]);
        if (n == 0) continue;
        BvhNode box;
        for (int a = 0; a < 3; ++a) { box.bmin[a] = lo[a]; box.bmax[a] = hi[a]; }
        for (size_t i = 1; i < n; ++i)
            for (int a = 0; a < 3; ++a) { box.bmin[a] = sel_min(box.bmin[a], lo[3 * i + a]); box.bmax[a] = sel_max(box.bmax[a], hi[3 * i + a]); }
        box.offset = 0; box.countAxis = 3u;
        objectBounds[o].nodes.push_back(box);
    }
    ComputePrimBounds(sc, objectBounds, &lo, &hi);
    const size_t n = lo.size() / 3;
    if (n > 0x3fffffffull) return SetError(HPRT_E_UNSUPPORTED, "more than 2^30 primitives");
    const std::string err = buildTree(-1, n, lo.data(), hi.data(), &t->top);
    if (!err.empty()) return SetError(HPRT_E_UNSUPPORTED, "top level: " + err);
    if (int rc = CheckTwoLevelDepth(*t)) return rc;
    *out = t.release();
    return HPRT_OK;
}
// hprt_rbspinst_build / hprt_rbspkdinst_build; p: the Accelerator line.  The device-assisted build (costFn) is not wired in.
template <typename Params>
int BuildRbspInst(const char *fn, const HprtModel *m, const Params *params, RbspParams p, HprtRbspInst **out) {
    if (out) *out = nullptr;
    if (!m || !out) return SetError(HPRT_E_INVALID, std::string(fn) + ": null argument");
    const SceneModel &sc = m->sc;
    if (sc.instances.empty())
        return SetError(HPRT_E_UNSUPPORTED, std::string(fn) + ": the model has no object instances; build its tree with hprt_rbsp_build / hprt_rbspkd_build");
    p.kdAware = std::is_same<Params, HprtRbspKdParams>::value;
    ApplyRbspParams(params, &p);
    if (p.nDirections != 3 && p.nDirections != 7 && p.nDirections != 9 && p.nDirections != 13)
        return SetError(HPRT_E_UNSUPPORTED, "nbDirections " + std::to_string(p.nDirections) + " is not supported (3, 7, 9 or 13)");
    std::unique_ptr<HprtRbspInst> t(new HprtRbspInst());
    t->kdAware = p.kdAware;
    std::vector<float> tri9;
    std::vector<uint8_t> isTri;
    return BuildTwoLevel(sc, std::move(t),
                         [&](int object, size_t n, const float *lo, const float *hi, RbspTree *r) {
                             RbspPrimTriangles(sc, object, n, &tri9, &isTri);
                             return BuildRbspTree(n, lo, hi, tri9.data(), isTri.data(), p, r);
                         },
                         [&](size_t n, const float *lo, const float *hi, RbspTree *r) {
                             r->nPrims = (uint32_t)n; r->M = (uint32_t)p.nDirections;
                             RbspDirections(r->M, &r->directions);
                             for (int a = 0; a < 3 && n; ++a) { r->bounds[a] = lo[a]; r->bounds[3 + a] = hi[a]; }
                         },
                         out);
}
// hprt_bsppaperinst_build / hprt_bsppaperkdinst_build; p: the Accelerator line.  Every tree is BuildBspPaperTree over RbspPrimTriangles'
// view of its primitives: an object's triangles by their object-space vertices, a sphere as isTri = 0.  On the top level an instance
// is a TransformedPrimitive, which inherits Primitive::getBSPPaperPlanes (core/primitive.h:92-95: no planes) and
// Primitive::getBounds (the 8 corners of its WorldBound): isTri = 0 again, so an instance contributes axis candidates only and is
// classified under a plane exactly as the builder classifies every other non-triangle.
template <typename Params>
int BuildBspPaperInst(const char *fn, const HprtModel *m, const Params *params, BspPaperParams p, HprtBspPaperInst **out) {
    constexpr bool kdAware = std::is_same<Params, HprtBspPaperKdParams>::value;
    if (out) *out = nullptr;
    if (!m || !out) return SetError(HPRT_E_INVALID, std::string(fn) + ": null argument");
    const SceneModel &sc = m->sc;
    if (sc.instances.empty())
        return SetError(HPRT_E_UNSUPPORTED, std::string(fn) + ": the model has no object instances; build its tree with hprt_bsppaper_build / hprt_bsppaperkd_build");
    p.kdAware = kdAware;
    if (params) {
        p.isectCost = params->isect_cost; p.travCost = params->trav_cost; p.emptyBonus = params->empty_bonus;
        p.maxPrims = params->max_prims; p.maxDepth = params->max_depth; p.threads = params->threads;
        if constexpr (kdAware) p.kdTravCost = params->kd_trav_cost;
    }
    std::unique_ptr<HprtBspPaperInst> t(new HprtBspPaperInst());
    t->kdAware = kdAware;
    t->top.kdAware = kdAware;
    std::vector<float> tri9;
    std::vector<uint8_t> isTri;
    return BuildTwoLevel(sc, std::move(t),
                         [&](int object, size_t n, const float *lo, const float *hi, BspPaperTree *b) {      // maxDepth -1 resolves per tree, from its n
                             if (n > (kdAware ? 0x0fffffffull : 0x3fffffffull)) return std::string("more primitives than a node's flags can count");
                             RbspPrimTriangles(sc, object, n, &tri9, &isTri);
                             return BuildBspPaperTree(n, lo, hi, tri9.data(), isTri.data(), p, b);
                         },
                         [&](size_t n, const float *lo, const float *hi, BspPaperTree *b) {
                             b->nPrims = (uint32_t)n; b->kdAware = kdAware;
                             for (int a = 0; a < 3 && n; ++a) { b->bounds[a] = lo[a]; b->bounds[3 + a] = hi[a]; }
                         },
                         out);
}
// hprt_bspnodeinst_build / hprt_bspnodeinst_build_device: the two-level form of the nine node-based trees.  Every tree is
// BuildBspNodeTree over RbspPrimTriangles' view of its primitives, from a fresh std::mt19937(seed) (which is what a BuildBspNodeTree
// call starts).  What the reference's builds call on a primitive is WorldBound, getBounds(d) and — through the choosers — Normal
// (bspNodeBased.cpp:34,124, bspNodeBasedFastKd.cpp:38,206, randomNormals.h:22, clustering.h:63); getSurfaceArea is reached by the
// debugging dump of genericBSP.h:107-130 alone.  On the top level an instance is a TransformedPrimitive (core/primitive.h:144-182):
// Normal() is (0, 0, 0) and getBounds is Primitive's over the 8 corners of its WorldBound — isTri = 0, as the builder already
// treats a sphere.  One hook (hook != NULL: the device-assisted build) serves every tree through one device session.
int BuildBspNodeInst(const char *fn, const HprtModel *m, const HprtBspNodeParams *params, HprtBspPaperInst **out, const BspNodeHook *hook = nullptr) {
    if (out) *out = nullptr;
    if (!m || !out) return SetError(HPRT_E_INVALID, std::string(fn) + ": null argument");
    const SceneModel &sc = m->sc;
    if (sc.instances.empty())
        return SetError(HPRT_E_UNSUPPORTED, std::string(fn) + ": the model has no object instances; build its tree with hprt_bspnode_build / hprt_bspnodekd_build");
    BspNodeParams p = sc.opt.bspnode;
    if (!params && !BspNodeAccelerator(sc.opt.accelerator, &p.chooser, &p.form))
        return SetError(HPRT_E_INVALID, std::string(fn) + ": the scene's Accelerator \"" + sc.opt.accelerator + "\" is no node-based BSP tree; pass params");
    ApplyBspNodeParams(params, &p);
    const std::string refused = BspNodeRefuseParams(p);      // before any primitive is looked at, and before a device is opened
    if (!refused.empty()) return SetError(HPRT_E_UNSUPPORTED, refused);
    const bool fastKd = p.form == BSPNODE_FASTKD;
    std::unique_ptr<HprtBspPaperInst> t(new HprtBspPaperInst());
    t->kdAware = fastKd;
    t->top.kdAware = fastKd;
    BspNodeHookState hs;                                 // (the device is freed when the build ends or fails)
    if (const int rc = hs.Install(hook, &p)) return rc;
    std::vector<float> tri9;
    std::vector<uint8_t> isTri;
    const int rc = BuildTwoLevel(sc, std::move(t),
                                 [&](int object, size_t n, const float *lo, const float *hi, BspPaperTree *b) {      // maxDepth -1 resolves per tree, from its n
                                     if (n > (fastKd ? 0x0fffffffull : 0x3fffffffull)) return std::string("more primitives than a node's flags can count");
                                     RbspPrimTriangles(sc, object, n, &tri9, &isTri);
                                     return BuildBspNodeTree(n, lo, hi, tri9.data(), isTri.data(), p, b);
                                 },
                                 [&](size_t n, const float *lo, const float *hi, BspPaperTree *b) {
                                     b->nPrims = (uint32_t)n; b->kdAware = fastKd;
                                     for (int a = 0; a < 3 && n; ++a) { b->bounds[a] = lo[a]; b->bounds[3 + a] = hi[a]; }
                                 },
                                 out);
    if (hook && hook->stats)
        *hook->stats = HprtBuildDeviceStats{hs.st.bs.nodesDevice, hs.st.bs.candidatesDevice, hs.st.bs.candidatesRecosted, hs.st.bs.nodesHost, hs.st.bs.secondsDevice};
    if (hs.st.rc != HPRT_OK) return SetError(hs.st.rc, g_lastError);      // the device's failure keeps its code under BuildTwoLevel's prefix
    return rc;
}
// info[0..3] of one tree of a handle: an object without a tree has no leaves and no depth
template <typename Tree>
void TwoLevelTreeInfo(const Tree &t, uint32_t info[4]) {
    info[0] = (uint32_t)t.nodes.size(); info[1] = t.nodes.empty() ? 0u : t.leaves; info[2] = (uint32_t)t.primIndices.size(); info[3] = t.nodes.empty() ? 0u : t.depth;
}
// info[0..7] of either handle
template <typename Handle>
int TwoLevelInfo(const char *fn, const Handle *t, uint32_t *info) {
    if (!t || !info) return SetError(HPRT_E_INVALID, std::string(fn) + ": null argument");
    TwoLevelTreeInfo(t->top, info);
    info[4] = (uint32_t)t->objects.size(); info[5] = 0; info[6] = 0; info[7] = (uint32_t)t->instanceObject.size();
    for (const auto &o : t->objects) if (!o.nodes.empty()) { ++info[5]; info[6] = std::max(info[6], o.depth); }
    return HPRT_OK;
}
// The tree of object definition `object` (object_info, object_copy); NULL with the error set when there is none
template <typename Handle>
auto TwoLevelObject(const char *fn, const Handle *t, uint32_t object) -> decltype(&t->top) {
    if (!t) SetError(HPRT_E_INVALID, std::string(fn) + ": null argument");
    else if (object >= t->objects.size()) SetError(HPRT_E_INVALID, std::string(fn) + ": object index out of range");
    else return &t->objects[object];
    return nullptr;
}
template <typename Handle>
int TwoLevelObjectInfo(const char *fn, const Handle *t, uint32_t object, uint32_t *info) {
    if (!t || !info) return SetError(HPRT_E_INVALID, std::string(fn) + ": null argument");
    const auto *o = TwoLevelObject(fn, t, object);
    if (!o) return HPRT_E_INVALID;
    TwoLevelTreeInfo(*o, info);
    return HPRT_OK;
}
// The diagnostics hooks hprt_debug_*_bounds and hprt_debug_*_set_tree (below)
template <typename Handle>
int TwoLevelBounds(const char *fn, const Handle *t, int object, float *bounds6) {
    if (!t || !bounds6 || object >= (int)t->objects.size()) return SetError(HPRT_E_INVALID, std::string(fn) + ": bad argument");
    memcpy(bounds6, (object < 0 ? t->top : t->objects[object]).bounds, 6 * sizeof(float));
    return HPRT_OK;
}
// What a hand-made tree keeps of the tree it replaces — its primitive count; an RBSP tree its M and direction table too — then its
// structural check, which gives its depth, and its leaves
const char *FinishHandMadeTree(const KdTree &old, KdTree *k) {
    k->nPrims = old.nPrims;
    k->leaves = CountLeaves(k->nodes, 3u, 3u);
    return CheckKdTree(*k, &k->depth);
}
const char *FinishHandMadeTree(const RbspTree &old, RbspTree *r) {
    r->nPrims = old.nPrims; r->M = old.M; r->directions = old.directions;
    r->leaves = CountLeaves(r->nodes, RbspBitMask(r->M), r->M);
    return CheckRbspTree(*r, &r->depth);
}
// a general BSP tree keeps its node layout; its axis / plane node counts are a hand-made tree's (CountHandMadeInterior)
const char *FinishHandMadeTree(const BspPaperTree &old, BspPaperTree *b) {
    b->nPrims = old.nPrims; b->kdAware = old.kdAware;
    const uint32_t mask = b->kdAware ? (uint32_t)BSPPAPERKD_MASK : (uint32_t)BSPPAPER_MASK, leafTag = b->kdAware ? (uint32_t)BSPPAPERKD_LEAF : 1u;
    b->leaves = CountLeaves(b->nodes, mask, leafTag);
    CountHandMadeInterior(b);
    return b->kdAware ? CheckBspPaperKdTree(*b, &b->depth) : CheckBspPaperTree(*b, &b->depth);
}
// The node words of a hand-made tree: 8 bytes per node, or (a general BSP tree) the 20 bytes BspPaperCopy writes, whose axes the
// 8-byte form cannot carry
void SetTreeNodes(KdTree *k, size_t nNodes, const uint32_t *nodes8) { k->nodes.resize(nNodes); memcpy(k->nodes.data(), nodes8, nNodes * sizeof(BspNode)); }
void SetTreeNodes(RbspTree *r, size_t nNodes, const uint32_t *nodes8) { r->nodes.resize(nNodes); memcpy(r->nodes.data(), nodes8, nNodes * sizeof(BspNode)); }
void SetTreeNodes(BspPaperTree *b, size_t nNodes, const uint32_t *nodes20) {
    b->nodes.resize(nNodes); b->axes.resize(3 * nNodes);
    for (size_t k = 0; k < nNodes; ++k) {
        b->nodes[k] = BspNode{nodes20[5 * k], nodes20[5 * k + 1]};
        memcpy(&b->axes[3 * k], &nodes20[5 * k + 2], 12);
    }
}
template <typename Handle>
int TwoLevelSetTree(const char *fn, Handle *t, int object, size_t nNodes, const uint32_t *nodes8, size_t nIdx, const uint32_t *idx, const float *bounds6) {
    if (!t || !nodes8 || !bounds6 || (nIdx && !idx) || object >= (int)t->objects.size()) return SetError(HPRT_E_INVALID, std::string(fn) + ": bad argument");
    auto &dst = object < 0 ? t->top : t->objects[object];
    if (object >= 0 && dst.nPrims < 2) return SetError(HPRT_E_INVALID, std::string(fn) + ": an object of one primitive has no tree");
    typename std::remove_reference<decltype(dst)>::type tree;
    SetTreeNodes(&tree, nNodes, nodes8);
    tree.primIndices.assign(idx, idx + nIdx);
    memcpy(tree.bounds, bounds6, sizeof(tree.bounds));
    const char *bad = FinishHandMadeTree(dst, &tree);
    if (*bad) return SetError(HPRT_E_INVALID, std::string("malformed tree: ") + bad);
    tree.maxDepth = tree.depth;
    std::swap(dst, tree);
    if (int rc = CheckTwoLevelDepth(*t)) { std::swap(dst, tree); return rc; }
    return HPRT_OK;
}

// Film::WriteGeneralStats (core/film.cpp:170-187) with WriteGeneralStatMatrix (:189-210): the eight matrices, each to
// "<prefix>-<name>.txt", one image row per line; value(k, i): matrix k's value at pixel i (row-major)
template <typename Value>
int WriteStatMatrices(const char *prefix, int width, int height, Value value) {
    static const char *const kNames[8] = {"primitiveIntersections", "primitiveIntersectionsP", "kdTreeNodeTraversals", "kdTreeNodeTraversalsP",
                                          "bspTreeNodeTraversals", "bspTreeNodeTraversalsP", "leafNodeTraversals", "leafNodeTraversalsP"};
    for (int k = 0; k < 8; ++k) {
        const std::string path = std::string(prefix) + "-" + kNames[k] + ".txt";
        FILE *fp = fopen(path.c_str(), "w");
        if (!fp) return SetError(HPRT_E_IO, "cannot create " + path);
        bool ok = true;
        for (int y = 0; y < height && ok; ++y) {
            for (int x = 0; x < width; ++x) {
                const unsigned long long v = value(k, (size_t)y * width + x);
                ok = ok && fprintf(fp, x ? " %llu" : "%llu", v) > 0;
            }
            ok = ok && fputc('\n', fp) != EOF;
        }
        if (fclose(fp) != 0) ok = false;
        if (!ok) return SetError(HPRT_E_IO, "write error on " + path);
    }
    return HPRT_OK;
}
// hprt_bsppaper*_build*_device and the diagnostics hooks: a model's primitives, or n triangles, through BuildBspPaper with a hook
template <typename Handle, typename Params>
int BuildBspPaperFromModel(const char *fn, const char *what, const HprtModel *m, const Params *params, Handle **out, const BspHook *hook) {
    if (!m || !out) return SetError(HPRT_E_INVALID, std::string(fn) + ": null argument");
    *out = nullptr;
    if (m->sc.nObjects != 0 || !m->sc.instances.empty())
        return SetError(HPRT_E_UNSUPPORTED, std::string(what) + " trees over object instances are not supported (the scene keeps its BVH)");
    std::vector<float> lo, hi, tri9;
    std::vector<uint8_t> isTri;
    RbspModelPrims(m, &lo, &hi, &tri9, &isTri);
    const BspPaperParams dflt = std::is_same<Handle, HprtBspPaperKd>::value ? m->sc.opt.bsppaperkd : m->sc.opt.bsppaper;
    return BuildBspPaper(lo.size() / 3, lo.data(), hi.data(), tri9.data(), isTri.data(), params, dflt, out, hook);
}
template <typename Handle, typename Params>
int BuildBspPaperFromTriangles(const char *fn, size_t n, const float *p9, const Params *params, Handle **out, const BspHook *hook) {
    if (!out || (n && !p9)) return SetError(HPRT_E_INVALID, std::string(fn) + ": null argument");
    *out = nullptr;
    constexpr bool kdAware = std::is_same<Handle, HprtBspPaperKd>::value;
    if (n > (kdAware ? 0x0fffffffull : 0x3fffffffull)) return SetError(HPRT_E_UNSUPPORTED, kdAware ? "more than 2^28 primitives" : "more than 2^30 primitives");
    std::vector<float> lo, hi;
    RbspTriangleBounds(n, p9, &lo, &hi);
    std::vector<uint8_t> isTri(n, 1);
    return BuildBspPaper(n, lo.data(), hi.data(), p9, isTri.data(), params, BspPaperParams(), out, hook);
}
}  // namespace

extern "C" {

const char *hprt_last_error(void) { return g_lastError.c_str(); }
const char *hprt_version(void) { return "hprt 0.1 gfx950 (HIP, wave64) host+device"; }

int hprt_model_parse(const char *pbrt_path, const char *const *subst, int n_subst, HprtModel **out) try {
    if (!pbrt_path || !out) return SetError(HPRT_E_INVALID, "hprt_model_parse: null argument");
    std::map<std::string, std::string> sm;
    sm["$acc"] = "\"bvh\"";
    for (int i = 0; i + 1 < 2 * n_subst; i += 2) if (subst && subst[i] && subst[i + 1]) sm[subst[i]] = subst[i + 1];
    HprtModel *m = new HprtModel();
    std::string err;
    if (!ParsePbrtFile(pbrt_path, sm, &m->sc, &err)) { delete m; return SetError(HPRT_E_PARSE, err); }
    // a tree over object instances is not built (hprt_<accelerator>_build: HPRT_E_UNSUPPORTED): such a scene keeps the BVH and the warning
    static const char *const kTreeAccelerators[] = {"kdtree", "rbsp", "rbspkd", "bsppaper", "bsppaperkd"};
    int nodeChooser, nodeForm;     // the node-based BSP trees: hprt_bspnode[kd]_build, attached as bsppaper / bsppaperkd trees
    const std::string &acc = m->sc.opt.accelerator;
    const bool plainScene = m->sc.nObjects == 0 && m->sc.instances.empty();
    if (BspNodeAccelerator(acc, &nodeChooser, &nodeForm) && plainScene) {
        const std::string as = nodeForm == BSPNODE_FASTKD ? "bsppaperkd" : "bsppaper";
        m->sc.warnings.push_back("Accelerator \"" + acc + "\": the host builds the tree (hprt_bspnode" + (nodeForm == BSPNODE_FASTKD ? "kd" : "") +
                                 "_build) and attaches it to the scene (hprt_scene_attach_" + as + "); a scene without it walks a BVH");
    } else if (std::count(std::begin(kTreeAccelerators), std::end(kTreeAccelerators), acc) && plainScene)
        m->sc.warnings.push_back("Accelerator \"" + acc + "\": the host builds the tree (hprt_" + acc + "_build) and attaches it to the scene (hprt_scene_attach_" +
                                 acc + "); a scene without it walks a BVH");
    else if (acc == "bvhold")      // (with or without object instances: hprt_bvhold_build builds every aggregate's tree)
        m->sc.warnings.push_back("Accelerator \"bvhold\": the host builds the tree (hprt_bvhold_build) and passes it to hprt_scene_create_from_model; "
                                 "hprt_bvh_build builds the fork's BVH");
    else if (acc != "bvh") m->sc.warnings.push_back("Accelerator \"" + acc + "\" is outside the hot-path scope; \"bvh\" used");
    if (m->sc.opt.integrator == "ambientocclusion")
        m->sc.warnings.push_back("Integrator \"ambientocclusion\": the host renders it with hprt_render_ao; hprt_render renders the path integrator");
    else if (m->sc.opt.integrator == "directlighting")
        m->sc.warnings.push_back("Integrator \"directlighting\": the host renders it with hprt_render_direct; hprt_render renders the path integrator");
    else if (m->sc.opt.integrator != "path") m->sc.warnings.push_back("Integrator \"" + m->sc.opt.integrator + "\" is outside the hot-path scope; \"path\" used");
    if (m->sc.opt.sampler != "halton") m->sc.warnings.push_back("Sampler \"" + m->sc.opt.sampler + "\" is outside the hot-path scope; \"halton\" used");
    *out = m;
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
int hprt_model_load(const char *baked_path, HprtModel **out) try {
    if (!baked_path || !out) return SetError(HPRT_E_INVALID, "hprt_model_load: null argument");
    HprtModel *m = new HprtModel();
    std::string err;
    if (!LoadBakedScene(baked_path, &m->sc, &err)) { delete m; return SetError(HPRT_E_IO, err); }
    *out = m;
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
int hprt_model_save(const HprtModel *m, const char *baked_path) try {
    if (!m || !baked_path) return SetError(HPRT_E_INVALID, "hprt_model_save: null argument");
    std::string err;
    if (!SaveBakedScene(m->sc, baked_path, &err)) return SetError(HPRT_E_IO, err);
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
int hprt_model_save_compact(const HprtModel *m, const char *baked_path) try {
    if (!m || !baked_path) return SetError(HPRT_E_INVALID, "hprt_model_save_compact: null argument");
    std::string err;
    if (!SaveBakedScene(m->sc, baked_path, &err, true)) return SetError(HPRT_E_IO, err);
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
void hprt_model_destroy(HprtModel *m) { delete m; }

int hprt_model_get_options(const HprtModel *m, HprtRenderOptions *o) try {
    if (!m || !o) return SetError(HPRT_E_INVALID, "hprt_model_get_options: null argument");
    const RenderOptions &p = m->sc.opt;
    o->xres = p.xres; o->yres = p.yres;
    memcpy(o->crop, p.crop, 16);
    memcpy(o->filter_radius, p.filterRadius, 8);
    o->film_scale = p.filmScale; o->max_sample_luminance = p.maxSampleLuminance;
    o->fov = p.fov; o->lens_radius = p.lensRadius; o->focal_distance = p.focalDistance;
    memcpy(o->screen_window, p.screenWindow, 16);
    memcpy(o->camera_to_world, p.cameraToWorld.m, 64); memcpy(o->world_to_camera, p.worldToCamera.m, 64);
    o->spp = p.spp; o->sample_pixel_center = p.samplePixelCenter;
    o->max_depth = p.maxDepth; o->rr_threshold = p.rrThreshold; o->light_strategy = p.lightStrategy;
    o->max_node_prims = p.maxNodePrims; o->isect_cost = p.isectCost; o->trav_cost = p.travCost;
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
int hprt_model_set_options(HprtModel *m, const HprtRenderOptions *o) try {
    if (!m || !o) return SetError(HPRT_E_INVALID, "hprt_model_set_options: null argument");
    if (o->xres <= 0 || o->yres <= 0 || o->spp <= 0) return SetError(HPRT_E_INVALID, "resolution and spp must be positive");
    RenderOptions &p = m->sc.opt;
    p.xres = o->xres; p.yres = o->yres;
    memcpy(p.crop, o->crop, 16);
    memcpy(p.filterRadius, o->filter_radius, 8);
    p.filmScale = o->film_scale; p.maxSampleLuminance = o->max_sample_luminance;
    p.fov = o->fov; p.lensRadius = o->lens_radius; p.focalDistance = o->focal_distance;
    memcpy(p.screenWindow, o->screen_window, 16);
    memcpy(p.cameraToWorld.m, o->camera_to_world, 64); memcpy(p.worldToCamera.m, o->world_to_camera, 64);
    p.spp = o->spp; p.samplePixelCenter = o->sample_pixel_center;
    p.maxDepth = o->max_depth; p.rrThreshold = o->rr_threshold; p.lightStrategy = o->light_strategy;
    p.maxNodePrims = o->max_node_prims; p.isectCost = o->isect_cost; p.travCost = o->trav_cost;
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
int hprt_model_counts(const HprtModel *m, uint64_t c[7]) try {
    if (!m || !c) return SetError(HPRT_E_INVALID, "hprt_model_counts: null argument");
    uint64_t tris = 0, spheres = 0;
    for (const ShapeDesc &s : m->sc.shapes) { if (s.kind == kTriangleMesh) tris += s.mesh.nTris(); else ++spheres; }
    c[0] = m->sc.shapes.size(); c[1] = tris + spheres; c[2] = tris; c[3] = spheres;
    c[4] = m->sc.materials.size(); c[5] = m->sc.lights.size(); c[6] = m->sc.textures.size();
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
int hprt_model_texture_info(const HprtModel *m, uint32_t texture, int32_t info[5], float *max_anisotropy) try {
    if (!m || !info || texture >= m->sc.textures.size()) return SetError(HPRT_E_INVALID, "hprt_model_texture_info: bad argument");
    const TextureDesc &t = m->sc.textures[texture];
    info[0] = (int32_t)t.levels.size(); info[1] = t.trilinear; info[2] = t.wrap; info[3] = t.levels[0].w; info[4] = t.levels[0].h;
    if (max_anisotropy) *max_anisotropy = t.maxAniso;
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
int hprt_model_texture_level(const HprtModel *m, uint32_t texture, uint32_t level, int32_t wh[2], float *rgb) try {
    if (!m || !wh || texture >= m->sc.textures.size() || level >= m->sc.textures[texture].levels.size())
        return SetError(HPRT_E_INVALID, "hprt_model_texture_level: bad argument");
    const MipLevel &l = m->sc.textures[texture].levels[level];
    wh[0] = l.w; wh[1] = l.h;
    if (rgb) memcpy(rgb, l.rgb.data(), 4 * l.rgb.size());
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
const char *hprt_model_warnings(const HprtModel *m) {
    static thread_local std::string buf;
    buf.clear();
    if (m) for (const std::string &w : m->sc.warnings) { buf += w; buf += '\n'; }
    return buf.c_str();
}

int hprt_bvh_build(const HprtModel *m, HprtBvh **out) try {
    if (!m || !out) return SetError(HPRT_E_INVALID, "hprt_bvh_build: null argument");
    std::vector<float> lo, hi;
    HprtBvh *b = new HprtBvh();
    b->objects.resize(m->sc.nObjects);
    for (uint32_t o = 0; o < m->sc.nObjects; ++o) {
        ComputeObjectPrimBounds(m->sc, (int)o, &lo, &hi);
        BuildBvh(lo.size() / 3, lo.data(), hi.data(), m->sc.opt.maxNodePrims, m->sc.opt.isectCost, m->sc.opt.travCost, &b->objects[o]);
    }
    ComputePrimBounds(m->sc, b->objects, &lo, &hi);
    BuildBvh(lo.size() / 3, lo.data(), hi.data(), m->sc.opt.maxNodePrims, m->sc.opt.isectCost, m->sc.opt.travCost, &b->tree);
    *out = b;
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
int hprt_bvh_build_from_bounds(size_t n, const float *bmin, const float *bmax, int maxNodePrims, int isectCost, int travCost,
                               HprtBvh **out) try {
    if (!out || (n && (!bmin || !bmax))) return SetError(HPRT_E_INVALID, "hprt_bvh_build_from_bounds: null argument");
    if (n > 0x7fffffffull) return SetError(HPRT_E_UNSUPPORTED, "more than 2^31 primitives");
    HprtBvh *b = new HprtBvh();
    BuildBvh(n, bmin, bmax, maxNodePrims, isectCost, travCost, &b->tree);
    *out = b;
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
void hprt_bvh_destroy(HprtBvh *b) { delete b; }

// ---- the stock BVH (Accelerator "bvhold"): BVHAccelOld, accelerators/bvhOld.cpp ----
namespace {
using HlbvhDevicePtr = DevicePtr<HlbvhDevice, HlbvhDeviceDestroy>;

// HprtBvhOldParams over the Accelerator line's (or the defaults'); HPRT_OK or HPRT_E_INVALID
int BvhOldParamsOf(const char *fn, const HprtBvhOldParams *params, BvhOldParams *p) {
    if (!params) return HPRT_OK;
    if (params->split_method < HPRT_BVHOLD_SAH || params->split_method > HPRT_BVHOLD_EQUAL)
        return SetError(HPRT_E_INVALID, std::string(fn) + ": split_method is not one of HPRT_BVHOLD_SAH, _HLBVH, _MIDDLE, _EQUAL");
    p->splitMethod = params->split_method; p->maxNodePrims = params->max_node_prims;
    return HPRT_OK;
}
// One aggregate's tree, on the host or (dev) through the device session; `what` names the aggregate in a refusal
int BuildBvhOldTree(size_t n, const float *lo, const float *hi, const BvhOldParams &p, HlbvhDevice *dev, HprtBvhOldDeviceStats *stats, const std::string &what,
                    BvhTree *out) {
    if (n > 0x7fffffffull) return SetError(HPRT_E_UNSUPPORTED, what + "more than 2^31 - 1 primitives");
    // bounds that are not finite: refused by both builds before a Morton code or a bucket is formed from them (the reference
    // would run into one of its checks, or convert a NaN to an integer)
    for (size_t i = 0; i < 3 * n; ++i)
        if (!std::isfinite(lo[i]) || !std::isfinite(hi[i]))
            return SetError(HPRT_E_UNSUPPORTED, what + "bvhold: the bounds of primitive " + std::to_string(i / 3) + " are not finite");
    if (dev) {
        if (n > kHlbvhMaxPrims) return SetError(HPRT_E_UNSUPPORTED, what + "more than 2^26 primitives: beyond what the device build's one-workgroup scan serves (hprt_bvhold_build builds such a tree)");
        std::string err;
        const int rc = HlbvhDeviceBuild(dev, n, lo, hi, p.maxNodePrims, out, stats, &err);
        return rc == HPRT_OK ? HPRT_OK : SetError(rc, what + err);
    }
    const std::string refused = BuildBvhOld(n, lo, hi, p, out);
    return refused.empty() ? HPRT_OK : SetError(HPRT_E_UNSUPPORTED, what + refused);
}
// BuildBvhOld where hprt_bvh_build calls BuildBvh: every object definition's aggregate (pbrtObjectInstance,
// core/api.cpp:1798-1806, same parameters), then the top level over TransformedPrimitive::WorldBound
int BuildBvhOldModel(const HprtModel *m, const BvhOldParams &p, HlbvhDevice *dev, HprtBvhOldDeviceStats *stats, HprtBvh **out) {
    std::vector<float> lo, hi;
    std::unique_ptr<HprtBvh> b(new HprtBvh());
    b->objects.resize(m->sc.nObjects);
    for (uint32_t o = 0; o < m->sc.nObjects; ++o) {
        ComputeObjectPrimBounds(m->sc, (int)o, &lo, &hi);
        if (const int rc = BuildBvhOldTree(lo.size() / 3, lo.data(), hi.data(), p, dev, stats, "object " + std::to_string(o) + ": ", &b->objects[o])) return rc;
    }
    ComputePrimBounds(m->sc, b->objects, &lo, &hi);
    if (const int rc = BuildBvhOldTree(lo.size() / 3, lo.data(), hi.data(), p, dev, stats, "", &b->tree)) return rc;
    *out = b.release();
    return HPRT_OK;
}
// The device entries' session: no device, then the split method and the capacity, then the ordinal
int OpenHlbvhDevice(const char *fn, const BvhOldParams &p, const HprtBvhOldDeviceOpts *opts, HlbvhDevicePtr *dev) {
    std::string err;
    int nDevices = 0;
    if (const int rc = HlbvhDeviceCount(&nDevices, &err)) return SetError(rc, err);
    if (p.splitMethod != BVHOLD_HLBVH)
        return SetError(HPRT_E_UNSUPPORTED, std::string(fn) + ": only split method \"hlbvh\" has a device build; hprt_bvhold_build builds \"sah\", \"middle\" and \"equal\"");
    HlbvhDevice *d = nullptr;
    const int rc = HlbvhDeviceCreate(opts ? opts->device : 0, opts ? opts->serial_treelet_max : 0u, &d, &err);
    dev->reset(d);
    return rc == HPRT_OK ? HPRT_OK : SetError(rc, err);
}
}  // namespace

int hprt_bvhold_build(const HprtModel *m, const HprtBvhOldParams *params, HprtBvh **out) try {
    if (out) *out = nullptr;
    if (!m || !out) return SetError(HPRT_E_INVALID, "hprt_bvhold_build: null argument");
    BvhOldParams p;
    p.splitMethod = m->sc.opt.bvhOldSplitMethod; p.maxNodePrims = m->sc.opt.bvhOldMaxNodePrims;
    if (const int rc = BvhOldParamsOf("hprt_bvhold_build", params, &p)) return rc;
    return BuildBvhOldModel(m, p, nullptr, nullptr, out);
} catch (...) { return hprt::HandleException(); }
int hprt_bvhold_build_from_bounds(size_t n, const float *bmin, const float *bmax, const HprtBvhOldParams *params, HprtBvh **out) try {
    if (out) *out = nullptr;
    if (!out || (n && (!bmin || !bmax))) return SetError(HPRT_E_INVALID, "hprt_bvhold_build_from_bounds: null argument");
    BvhOldParams p;
    if (const int rc = BvhOldParamsOf("hprt_bvhold_build_from_bounds", params, &p)) return rc;
    std::unique_ptr<HprtBvh> b(new HprtBvh());
    if (const int rc = BuildBvhOldTree(n, bmin, bmax, p, nullptr, nullptr, "", &b->tree)) return rc;
    *out = b.release();
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
int hprt_bvhold_build_device(const HprtModel *m, const HprtBvhOldParams *params, const HprtBvhOldDeviceOpts *opts, HprtBvhOldDeviceStats *stats,
                             HprtBvh **out) try {
    if (out) *out = nullptr;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!m || !out) return SetError(HPRT_E_INVALID, "hprt_bvhold_build_device: null argument");
    BvhOldParams p;
    p.splitMethod = m->sc.opt.bvhOldSplitMethod; p.maxNodePrims = m->sc.opt.bvhOldMaxNodePrims;
    if (const int rc = BvhOldParamsOf("hprt_bvhold_build_device", params, &p)) return rc;
    HlbvhDevicePtr dev;                                  // freed when the build ends or fails
    if (const int rc = OpenHlbvhDevice("hprt_bvhold_build_device", p, opts, &dev)) return rc;
    return BuildBvhOldModel(m, p, dev.get(), stats, out);
} catch (...) { return hprt::HandleException(); }
int hprt_bvhold_build_device_from_bounds(size_t n, const float *bmin, const float *bmax, const HprtBvhOldParams *params, const HprtBvhOldDeviceOpts *opts,
                                         HprtBvhOldDeviceStats *stats, HprtBvh **out) try {
    if (out) *out = nullptr;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!out || (n && (!bmin || !bmax))) return SetError(HPRT_E_INVALID, "hprt_bvhold_build_device_from_bounds: null argument");
    BvhOldParams p;
    if (const int rc = BvhOldParamsOf("hprt_bvhold_build_device_from_bounds", params, &p)) return rc;
    HlbvhDevicePtr dev;
    if (const int rc = OpenHlbvhDevice("hprt_bvhold_build_device_from_bounds", p, opts, &dev)) return rc;
    std::unique_ptr<HprtBvh> b(new HprtBvh());
    if (const int rc = BuildBvhOldTree(n, bmin, bmax, p, dev.get(), stats, "", &b->tree)) return rc;
    *out = b.release();
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }

// ---- kd-tree (Accelerator "kdtree") ----
static int FinishKdTree(HprtKdTree *t, HprtKdTree **out) {
    if (t->tree.depth > KD_TODO_MAX) {
        const std::string msg = TooDeepMessage("kd-tree", t->tree.depth, KD_TODO_MAX);
        delete t;
        return SetError(HPRT_E_UNSUPPORTED, msg);
    }
    *out = t;
    return HPRT_OK;
}
int hprt_model_accelerator(const HprtModel *m, char *name, size_t cap) try {
    if (!m || !name || cap == 0) return SetError(HPRT_E_INVALID, "hprt_model_accelerator: bad argument");
    const std::string &a = m->sc.opt.accelerator;
    if (a.size() + 1 > cap) return SetError(HPRT_E_INVALID, "hprt_model_accelerator: buffer too small");
    memcpy(name, a.c_str(), a.size() + 1);
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
int hprt_model_integrator(const HprtModel *m, char *name, size_t cap, HprtAoParams *ao) try {
    if (!m || !name || cap == 0) return SetError(HPRT_E_INVALID, "hprt_model_integrator: bad argument");
    const std::string &a = m->sc.opt.integrator;
    if (a.size() + 1 > cap) return SetError(HPRT_E_INVALID, "hprt_model_integrator: buffer too small");
    memcpy(name, a.c_str(), a.size() + 1);
    if (ao) { ao->n_samples = m->sc.opt.aoSamples; ao->cos_sample = m->sc.opt.aoCosSample; }
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
int hprt_model_direct(const HprtModel *m, HprtDirectParams *params, int32_t *n_light_samples, size_t cap, size_t *n_lights) try {
    if (!m || (cap && !n_light_samples)) return SetError(HPRT_E_INVALID, "hprt_model_direct: bad argument");
    if (params) { params->strategy = m->sc.opt.dlStrategy; params->max_depth = m->sc.opt.dlMaxDepth; }
    const size_t n = m->sc.lights.size();
    if (n_lights) *n_lights = n;
    // (a loaded model keeps no counts: they are not baked)
    for (size_t i = 0; i < n && i < cap; ++i) n_light_samples[i] = i < m->sc.lightSamples.size() ? m->sc.lightSamples[i] : 1;
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
int hprt_kdtree_build(const HprtModel *m, HprtKdTree **out) try {
    if (!m || !out) return SetError(HPRT_E_INVALID, "hprt_kdtree_build: null argument");
    if (m->sc.nObjects != 0 || !m->sc.instances.empty()) return SetError(HPRT_E_UNSUPPORTED, "kd-trees over object instances are not supported (the scene keeps its BVH)");
    std::vector<float> lo, hi;
    ComputePrimBounds(m->sc, {}, &lo, &hi);
    HprtKdTree *t = new HprtKdTree();
    BuildKdTree(lo.size() / 3, lo.data(), hi.data(), m->sc.opt.kd, &t->tree);
    return FinishKdTree(t, out);
} catch (...) { return hprt::HandleException(); }
int hprt_kdtree_build_from_bounds(size_t n, const float *bmin, const float *bmax, int isectCost, int travCost, float emptyBonus,
                                  int maxPrims, int maxDepth, HprtKdTree **out) try {
    if (!out || (n && (!bmin || !bmax))) return SetError(HPRT_E_INVALID, "hprt_kdtree_build_from_bounds: null argument");
    if (n > 0x3fffffffull) return SetError(HPRT_E_UNSUPPORTED, "more than 2^30 primitives");
    KdParams p;
    p.isectCost = isectCost; p.travCost = travCost; p.emptyBonus = emptyBonus; p.maxPrims = maxPrims; p.maxDepth = maxDepth;
    HprtKdTree *t = new HprtKdTree();
    BuildKdTree(n, bmin, bmax, p, &t->tree);
    return FinishKdTree(t, out);
} catch (...) { return hprt::HandleException(); }
int hprt_kdtree_info(const HprtKdTree *t, uint32_t info[4]) try {
    if (!t || !info) return SetError(HPRT_E_INVALID, "hprt_kdtree_info: null argument");
    info[0] = (uint32_t)t->tree.nodes.size(); info[1] = t->tree.leaves; info[2] = (uint32_t)t->tree.primIndices.size(); info[3] = t->tree.depth;
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
int hprt_kdtree_copy(const HprtKdTree *t, void *nodes8, uint32_t *primIndices) try {
    if (!t) return SetError(HPRT_E_INVALID, "hprt_kdtree_copy: null argument");
    if (nodes8) memcpy(nodes8, t->tree.nodes.data(), t->tree.nodes.size() * sizeof(KdNode));
    if (primIndices && !t->tree.primIndices.empty()) memcpy(primIndices, t->tree.primIndices.data(), t->tree.primIndices.size() * 4);
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
void hprt_kdtree_destroy(HprtKdTree *t) { delete t; }

// ---- two-level kd-trees (Accelerator "kdtree" over object instances, core/api.cpp:1794-1819; helpers above) ----
int hprt_kdinst_build(const HprtModel *m, HprtKdInst **out) try {
    if (!m || !out) return SetError(HPRT_E_INVALID, "hprt_kdinst_build: null argument");
    const SceneModel &sc = m->sc;
    if (sc.instances.empty())
        return SetError(HPRT_E_UNSUPPORTED, "hprt_kdinst_build: the model has no object instances; build its kd-tree with hprt_kdtree_build");
    return BuildTwoLevel(sc, std::unique_ptr<HprtKdInst>(new HprtKdInst()),
                         [&](int, size_t n, const float *lo, const float *hi, KdTree *k) { BuildKdTree(n, lo, hi, sc.opt.kd, k); return std::string(); },
                         [](size_t n, const float *, const float *, KdTree *k) { k->nPrims = (uint32_t)n; }, out);
} catch (...) { return hprt::HandleException(); }
static void KdTreeCopy(const KdTree &k, void *nodes8, uint32_t *primIndices) {
    if (nodes8 && !k.nodes.empty()) memcpy(nodes8, k.nodes.data(), k.nodes.size() * sizeof(KdNode));
    if (primIndices && !k.primIndices.empty()) memcpy(primIndices, k.primIndices.data(), k.primIndices.size() * 4);
}
int hprt_kdinst_info(const HprtKdInst *t, uint32_t info[8]) try {
    return TwoLevelInfo("hprt_kdinst_info", t, info);
} catch (...) { return hprt::HandleException(); }
int hprt_kdinst_object_info(const HprtKdInst *t, uint32_t object, uint32_t info[4]) try {
    return TwoLevelObjectInfo("hprt_kdinst_object_info", t, object, info);
} catch (...) { return hprt::HandleException(); }
int hprt_kdinst_copy(const HprtKdInst *t, void *nodes8, uint32_t *primIndices) try {
    if (!t) return SetError(HPRT_E_INVALID, "hprt_kdinst_copy: null argument");
    KdTreeCopy(t->top, nodes8, primIndices);
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
int hprt_kdinst_object_copy(const HprtKdInst *t, uint32_t object, void *nodes8, uint32_t *primIndices) try {
    const KdTree *o = TwoLevelObject("hprt_kdinst_object_copy", t, object);
    if (!o) return HPRT_E_INVALID;
    KdTreeCopy(*o, nodes8, primIndices);
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
void hprt_kdinst_destroy(HprtKdInst *t) { delete t; }
// Diagnostics hooks (not part of include/hprt.h; tests): the bounds of the top-level tree (object < 0) or of one object's tree, and
// a tree made by hand in place of the built one — nodes8 / idx as hprt_kdinst_copy writes them, bounds6 pMin then pMax — so that
// trees with a known todo depth reach the walk.  The tree keeps its primitive count and passes the structural check and the
// two-level depth rule a built handle passes (HPRT_E_INVALID, HPRT_E_UNSUPPORTED; the handle is unchanged when refused).
__attribute__((visibility("default"))) int hprt_debug_kdinst_bounds(const HprtKdInst *t, int object, float bounds6[6]) try {
    return TwoLevelBounds("hprt_debug_kdinst_bounds", t, object, bounds6);
} catch (...) { return hprt::HandleException(); }
__attribute__((visibility("default"))) int hprt_debug_kdinst_set_tree(HprtKdInst *t, int object, size_t n_nodes, const uint32_t *nodes8, size_t n_idx,
                                                                       const uint32_t *idx, const float *bounds6) try {
    return TwoLevelSetTree("hprt_debug_kdinst_set_tree", t, object, n_nodes, nodes8, n_idx, idx, bounds6);
} catch (...) { return hprt::HandleException(); }

// ---- RBSP tree (Accelerator "rbsp") and kd-aware RBSP tree (Accelerator "rbspkd"): one RbspTree, two handle types (helpers above) ----
int hprt_rbsp_build(const HprtModel *m, const HprtRbspParams *params, HprtRbsp **out) try {
    return BuildRbspFromModel("hprt_rbsp_build", "RBSP", m, params, m ? m->sc.opt.rbsp : RbspParams(), out);
} catch (...) { return hprt::HandleException(); }
int hprt_rbsp_build_from_triangles(size_t n, const float *p9, const HprtRbspParams *params, HprtRbsp **out) try {
    return BuildRbspFromTriangles("hprt_rbsp_build_from_triangles", n, p9, params, out);
} catch (...) { return hprt::HandleException(); }
int hprt_rbsp_info(const HprtRbsp *t, uint32_t info[5]) try {
    return RbspInfo("hprt_rbsp_info", t ? &t->tree : nullptr, info, false);
} catch (...) { return hprt::HandleException(); }
int hprt_rbsp_copy(const HprtRbsp *t, void *nodes8, uint32_t *primIndices, float *directions) try {
    return RbspCopy("hprt_rbsp_copy", t ? &t->tree : nullptr, nodes8, primIndices, directions);
} catch (...) { return hprt::HandleException(); }
void hprt_rbsp_destroy(HprtRbsp *t) { delete t; }
int hprt_rbspkd_build(const HprtModel *m, const HprtRbspKdParams *params, HprtRbspKd **out) try {
    return BuildRbspFromModel("hprt_rbspkd_build", "rbspkd", m, params, m ? m->sc.opt.rbspkd : RbspParams(), out);
} catch (...) { return hprt::HandleException(); }
int hprt_rbspkd_build_from_triangles(size_t n, const float *p9, const HprtRbspKdParams *params, HprtRbspKd **out) try {
    return BuildRbspFromTriangles("hprt_rbspkd_build_from_triangles", n, p9, params, out);
} catch (...) { return hprt::HandleException(); }
int hprt_rbspkd_info(const HprtRbspKd *t, uint32_t info[7]) try {
    return RbspInfo("hprt_rbspkd_info", t ? &t->tree : nullptr, info, true);
} catch (...) { return hprt::HandleException(); }
int hprt_rbspkd_copy(const HprtRbspKd *t, void *nodes8, uint32_t *primIndices, float *directions) try {
    return RbspCopy("hprt_rbspkd_copy", t ? &t->tree : nullptr, nodes8, primIndices, directions);
} catch (...) { return hprt::HandleException(); }
void hprt_rbspkd_destroy(HprtRbspKd *t) { delete t; }
// ---- the device-assisted builds: the same builder with its candidates costed by k_kdopcost (device/kdop_cost.hip) ----
// ---- two-level RBSP trees (Accelerator "rbsp" / "rbspkd" over object instances; helpers above) ----
int hprt_rbspinst_build(const HprtModel *m, const HprtRbspParams *params, HprtRbspInst **out) try {
    return BuildRbspInst("hprt_rbspinst_build", m, params, m ? m->sc.opt.rbsp : RbspParams(), out);
} catch (...) { return hprt::HandleException(); }
int hprt_rbspkdinst_build(const HprtModel *m, const HprtRbspKdParams *params, HprtRbspInst **out) try {
    return BuildRbspInst("hprt_rbspkdinst_build", m, params, m ? m->sc.opt.rbspkd : RbspParams(), out);
} catch (...) { return hprt::HandleException(); }
int hprt_rbspinst_info(const HprtRbspInst *t, uint32_t info[10]) try {
    if (int rc = TwoLevelInfo("hprt_rbspinst_info", t, info)) return rc;
    info[8] = t->top.M; info[9] = t->kdAware ? 1u : 0u;
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
int hprt_rbspinst_object_info(const HprtRbspInst *t, uint32_t object, uint32_t info[4]) try {
    return TwoLevelObjectInfo("hprt_rbspinst_object_info", t, object, info);
} catch (...) { return hprt::HandleException(); }
int hprt_rbspinst_copy(const HprtRbspInst *t, void *nodes8, uint32_t *primIndices, float *directions) try {
    return RbspCopy("hprt_rbspinst_copy", t ? &t->top : nullptr, nodes8, primIndices, directions);
} catch (...) { return hprt::HandleException(); }
int hprt_rbspinst_object_copy(const HprtRbspInst *t, uint32_t object, void *nodes8, uint32_t *primIndices) try {
    const RbspTree *o = TwoLevelObject("hprt_rbspinst_object_copy", t, object);
    if (!o) return HPRT_E_INVALID;
    return RbspCopy("hprt_rbspinst_object_copy", o, nodes8, primIndices, nullptr);
} catch (...) { return hprt::HandleException(); }
void hprt_rbspinst_destroy(HprtRbspInst *t) { delete t; }
// Diagnostics hooks (not part of include/hprt.h; tests): the bounds of the top-level tree (object < 0) or of one object's tree, and
// a tree made by hand in place of the built one — nodes8 / idx as hprt_rbspinst_copy writes them, bounds6 pMin then pMax — so that
// trees with a known todo depth reach the walk.  The tree keeps its primitive count, M and direction table and passes the
// structural check and the two-level depth rule a built handle passes (HPRT_E_INVALID, HPRT_E_UNSUPPORTED; the handle is unchanged
// when refused).
__attribute__((visibility("default"))) int hprt_debug_rbspinst_bounds(const HprtRbspInst *t, int object, float bounds6[6]) try {
    return TwoLevelBounds("hprt_debug_rbspinst_bounds", t, object, bounds6);
} catch (...) { return hprt::HandleException(); }
__attribute__((visibility("default"))) int hprt_debug_rbspinst_set_tree(HprtRbspInst *t, int object, size_t n_nodes, const uint32_t *nodes8, size_t n_idx,
                                                                         const uint32_t *idx, const float *bounds6) try {
    return TwoLevelSetTree("hprt_debug_rbspinst_set_tree", t, object, n_nodes, nodes8, n_idx, idx, bounds6);
} catch (...) { return hprt::HandleException(); }

int hprt_rbsp_build_device(const HprtModel *m, const HprtRbspParams *params, const HprtBuildDeviceOpts *opts, HprtBuildDeviceStats *stats, HprtRbsp **out) try {
    RbspHook h; h.device = true; h.opts = opts; h.stats = stats;
    return BuildRbspFromModel("hprt_rbsp_build_device", "RBSP", m, params, m ? m->sc.opt.rbsp : RbspParams(), out, &h);
} catch (...) { return hprt::HandleException(); }
int hprt_rbsp_build_from_triangles_device(size_t n, const float *p9, const HprtRbspParams *params, const HprtBuildDeviceOpts *opts, HprtBuildDeviceStats *stats,
                                          HprtRbsp **out) try {
    RbspHook h; h.device = true; h.opts = opts; h.stats = stats;
    return BuildRbspFromTriangles("hprt_rbsp_build_from_triangles_device", n, p9, params, out, &h);
} catch (...) { return hprt::HandleException(); }
int hprt_rbspkd_build_device(const HprtModel *m, const HprtRbspKdParams *params, const HprtBuildDeviceOpts *opts, HprtBuildDeviceStats *stats, HprtRbspKd **out) try {
    RbspHook h; h.device = true; h.opts = opts; h.stats = stats;
    return BuildRbspFromModel("hprt_rbspkd_build_device", "rbspkd", m, params, m ? m->sc.opt.rbspkd : RbspParams(), out, &h);
} catch (...) { return hprt::HandleException(); }
int hprt_rbspkd_build_from_triangles_device(size_t n, const float *p9, const HprtRbspKdParams *params, const HprtBuildDeviceOpts *opts,
                                            HprtBuildDeviceStats *stats, HprtRbspKd **out) try {
    RbspHook h; h.device = true; h.opts = opts; h.stats = stats;
    return BuildRbspFromTriangles("hprt_rbspkd_build_from_triangles_device", n, p9, params, out, &h);
} catch (...) { return hprt::HandleException(); }

// ---- general BSP tree (Accelerator "bsppaper"; helpers above) ----
int hprt_bsppaper_build(const HprtModel *m, const HprtBspPaperParams *params, HprtBspPaper **out) try {
    if (!m || !out) return SetError(HPRT_E_INVALID, "hprt_bsppaper_build: null argument");
    if (m->sc.nObjects != 0 || !m->sc.instances.empty())
        return SetError(HPRT_E_UNSUPPORTED, "bsppaper trees over object instances are not supported (the scene keeps its BVH)");
    std::vector<float> lo, hi, tri9;
    std::vector<uint8_t> isTri;
    RbspModelPrims(m, &lo, &hi, &tri9, &isTri);
    return BuildBspPaper(lo.size() / 3, lo.data(), hi.data(), tri9.data(), isTri.data(), params, m->sc.opt.bsppaper, out);
} catch (...) { return hprt::HandleException(); }
int hprt_bsppaper_build_from_triangles(size_t n, const float *p9, const HprtBspPaperParams *params, HprtBspPaper **out) try {
    if (!out || (n && !p9)) return SetError(HPRT_E_INVALID, "hprt_bsppaper_build_from_triangles: null argument");
    if (n > 0x3fffffffull) return SetError(HPRT_E_UNSUPPORTED, "more than 2^30 primitives");
    std::vector<float> lo, hi;
    RbspTriangleBounds(n, p9, &lo, &hi);
    std::vector<uint8_t> isTri(n, 1);
    return BuildBspPaper(n, lo.data(), hi.data(), p9, isTri.data(), params, BspPaperParams(), out);
} catch (...) { return hprt::HandleException(); }
int hprt_bsppaper_info(const HprtBspPaper *t, uint32_t info[6]) try {
    if (!t || !info) return SetError(HPRT_E_INVALID, "hprt_bsppaper_info: null argument");
    const BspPaperTree &b = t->tree;
    info[0] = (uint32_t)b.nodes.size(); info[1] = b.leaves; info[2] = b.depth; info[3] = (uint32_t)b.primIndices.size();
    info[4] = b.axisNodes; info[5] = b.planeNodes;
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
int hprt_bsppaper_copy(const HprtBspPaper *t, void *nodes20, uint32_t *primIndices) try {
    if (!t) return SetError(HPRT_E_INVALID, "hprt_bsppaper_copy: null argument");
    return BspPaperCopy(t->tree, nodes20, primIndices);
} catch (...) { return hprt::HandleException(); }
void hprt_bsppaper_destroy(HprtBspPaper *t) { delete t; }

// ---- kd-aware general BSP tree (Accelerator "bsppaperkd"): the same BspPaperTree with BSPKdNode's flags, a handle type of its own ----
int hprt_bsppaperkd_build(const HprtModel *m, const HprtBspPaperKdParams *params, HprtBspPaperKd **out) try {
    if (!m || !out) return SetError(HPRT_E_INVALID, "hprt_bsppaperkd_build: null argument");
    if (m->sc.nObjects != 0 || !m->sc.instances.empty())
        return SetError(HPRT_E_UNSUPPORTED, "bsppaperkd trees over object instances are not supported (the scene keeps its BVH)");
    std::vector<float> lo, hi, tri9;
    std::vector<uint8_t> isTri;
    RbspModelPrims(m, &lo, &hi, &tri9, &isTri);
    return BuildBspPaper(lo.size() / 3, lo.data(), hi.data(), tri9.data(), isTri.data(), params, m->sc.opt.bsppaperkd, out);
} catch (...) { return hprt::HandleException(); }
int hprt_bsppaperkd_build_from_triangles(size_t n, const float *p9, const HprtBspPaperKdParams *params, HprtBspPaperKd **out) try {
    if (!out || (n && !p9)) return SetError(HPRT_E_INVALID, "hprt_bsppaperkd_build_from_triangles: null argument");
    if (n > 0x0fffffffull) return SetError(HPRT_E_UNSUPPORTED, "more than 2^28 primitives");
    std::vector<float> lo, hi;
    RbspTriangleBounds(n, p9, &lo, &hi);
    std::vector<uint8_t> isTri(n, 1);
    return BuildBspPaper(n, lo.data(), hi.data(), p9, isTri.data(), params, BspPaperParams(), out);
} catch (...) { return hprt::HandleException(); }
int hprt_bsppaperkd_info(const HprtBspPaperKd *t, uint32_t info[6]) try {
    if (!t || !info) return SetError(HPRT_E_INVALID, "hprt_bsppaperkd_info: null argument");
    const BspPaperTree &b = t->tree;
    info[0] = (uint32_t)b.nodes.size(); info[1] = b.leaves; info[2] = b.depth; info[3] = (uint32_t)b.primIndices.size();
    info[4] = b.axisNodes; info[5] = b.planeNodes;
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
int hprt_bsppaperkd_copy(const HprtBspPaperKd *t, void *nodes20, uint32_t *primIndices) try {
    if (!t) return SetError(HPRT_E_INVALID, "hprt_bsppaperkd_copy: null argument");
    return BspPaperCopy(t->tree, nodes20, primIndices);
} catch (...) { return hprt::HandleException(); }
void hprt_bsppaperkd_destroy(HprtBspPaperKd *t) { delete t; }
// ---- the device-assisted builds: the same builder with its candidates costed by k_bspcost (device/bsp_cost.hip) ----
int hprt_bsppaper_build_device(const HprtModel *m, const HprtBspPaperParams *params, const HprtBspBuildDeviceOpts *opts, HprtBuildDeviceStats *stats,
                               HprtBspPaper **out) try {
    BspHook h; h.device = true; h.opts = opts; h.stats = stats;
    return BuildBspPaperFromModel("hprt_bsppaper_build_device", "bsppaper", m, params, out, &h);
} catch (...) { return hprt::HandleException(); }
int hprt_bsppaper_build_from_triangles_device(size_t n, const float *p9, const HprtBspPaperParams *params, const HprtBspBuildDeviceOpts *opts,
                                              HprtBuildDeviceStats *stats, HprtBspPaper **out) try {
    BspHook h; h.device = true; h.opts = opts; h.stats = stats;
    return BuildBspPaperFromTriangles("hprt_bsppaper_build_from_triangles_device", n, p9, params, out, &h);
} catch (...) { return hprt::HandleException(); }
int hprt_bsppaperkd_build_device(const HprtModel *m, const HprtBspPaperKdParams *params, const HprtBspBuildDeviceOpts *opts, HprtBuildDeviceStats *stats,
                                 HprtBspPaperKd **out) try {
    BspHook h; h.device = true; h.opts = opts; h.stats = stats;
    return BuildBspPaperFromModel("hprt_bsppaperkd_build_device", "bsppaperkd", m, params, out, &h);
} catch (...) { return hprt::HandleException(); }
int hprt_bsppaperkd_build_from_triangles_device(size_t n, const float *p9, const HprtBspPaperKdParams *params, const HprtBspBuildDeviceOpts *opts,
                                                HprtBuildDeviceStats *stats, HprtBspPaperKd **out) try {
    BspHook h; h.device = true; h.opts = opts; h.stats = stats;
    return BuildBspPaperFromTriangles("hprt_bsppaperkd_build_from_triangles_device", n, p9, params, out, &h);
} catch (...) { return hprt::HandleException(); }
// Diagnostics hooks of the general BSP candidate costing (not part of include/hprt.h; tests/bsp_cost_nodes.py).
// hprt_debug_bsp_root_nodes hands out the first max_nodes nodes a build costs, in build order: mesh, directions, candidates, the
// BVH over the node's primitives and the build's primitive arrays, with the costs and (in the candidates) the counts the builder's
// own code gave them.  m != NULL: the model's primitives; else n triangles.  params: HprtBspPaperKdParams for both trees
// (kd_trav_cost is not read when kd_aware is 0).  The pointers are valid during the call only.
__attribute__((visibility("default"))) int hprt_debug_bsp_root_nodes(const HprtModel *m, size_t n, const float *p9, int kd_aware, const HprtBspPaperKdParams *params,
                                                                      uint32_t max_nodes, BspNodeSink sink, void *user) try {
    if (!params || !sink) return SetError(HPRT_E_INVALID, "hprt_debug_bsp_root_nodes: null argument");
    BspHook h; h.sink = sink; h.user = user; h.maxNodes = max_nodes;
    int rc;
    if (kd_aware) {
        HprtBspPaperKd *t = nullptr;
        rc = m ? BuildBspPaperFromModel("hprt_debug_bsp_root_nodes", "bsppaperkd", m, params, &t, &h)
               : BuildBspPaperFromTriangles("hprt_debug_bsp_root_nodes", n, p9, params, &t, &h);
        delete t;
    } else {
        const HprtBspPaperParams q{params->isect_cost, params->trav_cost, params->empty_bonus, params->max_prims, params->max_depth, params->threads};
        HprtBspPaper *t = nullptr;
        rc = m ? BuildBspPaperFromModel("hprt_debug_bsp_root_nodes", "bsppaper", m, &q, &t, &h)
               : BuildBspPaperFromTriangles("hprt_debug_bsp_root_nodes", n, p9, &q, &t, &h);
        delete t;
    }
    return rc;
} catch (...) { return hprt::HandleException(); }
// hprt_debug_bsp_cost costs a node again with impl 0 (the vector code of bsp_build.h plus NodeBvh::count, BspCostVector), 1
// (bsp_cost.h on the host) or 2 (k_bspcost).  nd: a node as the sink above receives it (costs / costs_fixed are not read; the
// scalars' four capacity fields may lower the compiled capacities).  counts: nBelow, nAbove per candidate (an axis candidate's and
// an out-of-extent plane's are the input's).  Everything the costing indexes by is checked first (HPRT_E_INVALID): M, every face
// id, the order and kind of the candidates, the BVH's structure, primOrder, primNums and the capacities.  A node that impl 1 / 2
// decline whole (its own mesh, faces or direction list beyond a capacity) comes back with every candidate flagged.
__attribute__((visibility("default"))) int hprt_debug_bsp_cost(const HprtDebugBspNode *nd, int kd_aware, int impl, float *costs, float *costs_fixed,
                                                                uint32_t *counts, uint8_t *overflow) try {
    using namespace bspcost;
    const char *fn = "hprt_debug_bsp_cost: ";
    if (!nd || !costs || !costs_fixed || !counts || !overflow || !nd->scalars || !nd->dirs || (nd->n && !nd->cands) || (nd->n_edges && !nd->edges))
        return SetError(HPRT_E_INVALID, std::string(fn) + "null argument");
    if (impl < 0 || impl > 2) return SetError(HPRT_E_INVALID, std::string(fn) + "impl is not 0, 1 or 2");
    if (nd->M == 0 || nd->M > 65536u || nd->n_edges > 65536u || nd->n > 0x7fffffffull || nd->n_total > 0x7fffffffull || nd->n_axis > nd->n)
        return SetError(HPRT_E_INVALID, std::string(fn) + "a size that cannot be real");
    Scalars sc;
    memcpy(&sc, nd->scalars, sizeof(sc));
    uint32_t cap[4];
    if (!Capacities(sc, cap)) return SetError(HPRT_E_INVALID, std::string(fn) + "a capacity field may only lower the compiled capacity");
    std::vector<Edge> mesh(nd->n_edges);
    if (nd->n_edges) memcpy(static_cast<void *>(mesh.data()), nd->edges, (size_t)nd->n_edges * sizeof(Edge));
    for (const Edge &e : mesh)
        if (e.f1 >= 2 * nd->M || e.f2 >= 2 * nd->M) return SetError(HPRT_E_INVALID, std::string(fn) + "a face id is not below 2 M");
    std::vector<Cand> cs(nd->n);
    if (nd->n) memcpy(static_cast<void *>(cs.data()), nd->cands, nd->n * sizeof(Cand));
    for (size_t k = 0; k < nd->n; ++k)
        if (k < nd->n_axis ? cs[k].k >= 3u : cs[k].k != 33u)
            return SetError(HPRT_E_INVALID, std::string(fn) + "the candidates are not n_axis axis candidates followed by plane candidates");
    std::vector<BvhNode> bvhNodes;
    std::vector<BvhRec> recs;
    if (nd->n_axis < nd->n) {
        if (!nd->bvh_nodes || !nd->prim_order || !nd->prim_nums || !nd->bmin || !nd->bmax || !nd->tri9 || !nd->is_tri || nd->n_bvh == 0 || nd->n_prims == 0 ||
            nd->n_bvh > 0x7fffffffu)
            return SetError(HPRT_E_INVALID, std::string(fn) + "plane candidates without a BVH or without primitives");
        bvhNodes.resize(nd->n_bvh);
        memcpy(static_cast<void *>(bvhNodes.data()), nd->bvh_nodes, (size_t)nd->n_bvh * sizeof(BvhNode));
        const char *bad = CheckBvhNodes(bvhNodes.data(), nd->n_bvh, nd->n_prims, nullptr);
        if (*bad) return SetError(HPRT_E_INVALID, std::string(fn) + "malformed BVH: " + bad);
        for (uint32_t i = 0; i < nd->n_prims; ++i)
            if (nd->prim_order[i] >= nd->n_prims || nd->prim_nums[i] >= nd->n_total)
                return SetError(HPRT_E_INVALID, std::string(fn) + "primOrder or primNums points outside the primitives");
        recs.resize(nd->n_bvh);
        BspBvhRecords(bvhNodes.data(), bvhNodes.size(), recs.data());
    }
    for (size_t k = 0; k < nd->n; ++k) { costs[k] = 0; costs_fixed[k] = std::numeric_limits<float>::infinity(); overflow[k] = 1; counts[2 * k] = cs[k].nBelow; counts[2 * k + 1] = cs[k].nAbove; }
    const BspCostRequest rq{mesh.data(), nd->n_edges, nd->dirs, nd->M, kd_aware != 0, sc, cs.data(), nd->n, nd->n_axis, bvhNodes.data(), recs.data(),
                            (uint32_t)recs.size(), nd->prim_order, nd->prim_nums, recs.empty() ? 0u : nd->n_prims, nd->bmin, nd->bmax, nd->tri9, nd->is_tri,
                            nd->n_total, costs, costs_fixed, overflow};
    int rc = 0;
    if (impl == 0) BspCostVector(rq);
    else if (impl == 1) rc = BspCostRestated(rq);
    else {
        std::string err;
        const uint32_t asked[4] = {sc.maxEdges, sc.maxFaces, sc.maxFaceEdges, sc.maxStack};
        BspCostDevice *d = nullptr;
        int drc = BspCostDeviceCreate(0, asked, nd->n_total, nd->bmin, nd->bmax, nd->tri9, nd->is_tri, &d, &err);
        const BspDevicePtr dev(d);
        if (drc != HPRT_OK) return SetError(drc, err);
        rc = BspCostOnDevice(d, cap, rq, &drc, &err);
        if (rc < 0) return SetError(drc, err);
    }
    if (rc == 1) return HPRT_OK;            // declined whole: every candidate flagged
    for (size_t k = 0; k < nd->n; ++k)
        if (!overflow[k]) { counts[2 * k] = cs[k].nBelow; counts[2 * k + 1] = cs[k].nAbove; }
        else { costs[k] = 0; costs_fixed[k] = std::numeric_limits<float>::infinity(); }
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
// ---- two-level general BSP trees (Accelerator "bsppaper" / "bsppaperkd" over object instances, pbrtObjectInstance,
// core/api.cpp:1794-1819: MakeAccelerator for every object of more than one primitive and again in pbrtWorldEnd; helpers above) ----
int hprt_bsppaperinst_build(const HprtModel *m, const HprtBspPaperParams *params, HprtBspPaperInst **out) try {
    return BuildBspPaperInst("hprt_bsppaperinst_build", m, params, m ? m->sc.opt.bsppaper : BspPaperParams(), out);
} catch (...) { return hprt::HandleException(); }
int hprt_bsppaperkdinst_build(const HprtModel *m, const HprtBspPaperKdParams *params, HprtBspPaperInst **out) try {
    return BuildBspPaperInst("hprt_bsppaperkdinst_build", m, params, m ? m->sc.opt.bsppaperkd : BspPaperParams(), out);
} catch (...) { return hprt::HandleException(); }
int hprt_bsppaperinst_info(const HprtBspPaperInst *t, uint32_t info[12]) try {
    if (int rc = TwoLevelInfo("hprt_bsppaperinst_info", t, info)) return rc;
    info[8] = t->kdAware ? 1u : 0u; info[9] = t->top.axisNodes; info[10] = t->top.planeNodes; info[11] = 0;
    for (const BspPaperTree &o : t->objects) if (!o.nodes.empty()) { info[9] += o.axisNodes; info[10] += o.planeNodes; }
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
int hprt_bsppaperinst_object_info(const HprtBspPaperInst *t, uint32_t object, uint32_t info[4]) try {
    return TwoLevelObjectInfo("hprt_bsppaperinst_object_info", t, object, info);
} catch (...) { return hprt::HandleException(); }
int hprt_bsppaperinst_copy(const HprtBspPaperInst *t, void *nodes20, uint32_t *primIndices) try {
    if (!t) return SetError(HPRT_E_INVALID, "hprt_bsppaperinst_copy: null argument");
    return BspPaperCopy(t->top, nodes20, primIndices);
} catch (...) { return hprt::HandleException(); }
int hprt_bsppaperinst_object_copy(const HprtBspPaperInst *t, uint32_t object, void *nodes20, uint32_t *primIndices) try {
    const BspPaperTree *o = TwoLevelObject("hprt_bsppaperinst_object_copy", t, object);
    if (!o) return HPRT_E_INVALID;
    return BspPaperCopy(*o, nodes20, primIndices);
} catch (...) { return hprt::HandleException(); }
void hprt_bsppaperinst_destroy(HprtBspPaperInst *t) { delete t; }
// Diagnostics hooks (not part of include/hprt.h; tests): the bounds of the top-level tree (object < 0) or of one object's tree, and
// a tree made by hand in place of the built one — nodes20 / idx as hprt_bsppaperinst_copy writes them (5 words per node: the 8-byte
// form cannot carry the axes), bounds6 pMin then pMax — so that trees with a known todo depth reach the walk.  The tree keeps its
// primitive count and node layout and passes the structural check (CheckBspPaperTree / CheckBspPaperKdTree) and the two-level depth
// rule a built handle passes (HPRT_E_INVALID, HPRT_E_UNSUPPORTED; the handle is unchanged when refused).
__attribute__((visibility("default"))) int hprt_debug_bsppaperinst_bounds(const HprtBspPaperInst *t, int object, float bounds6[6]) try {
    return TwoLevelBounds("hprt_debug_bsppaperinst_bounds", t, object, bounds6);
} catch (...) { return hprt::HandleException(); }
__attribute__((visibility("default"))) int hprt_debug_bsppaperinst_set_tree(HprtBspPaperInst *t, int object, size_t n_nodes, const uint32_t *nodes20, size_t n_idx,
                                                                             const uint32_t *idx, const float *bounds6) try {
    return TwoLevelSetTree("hprt_debug_bsppaperinst_set_tree", t, object, n_nodes, nodes20, n_idx, idx, bounds6);
} catch (...) { return hprt::HandleException(); }
// ---- node-based BSP trees (Accelerator "bsparbitrary", "bspcluster", "bsprandom" and their withkd / fastkd forms; helpers above):
// no handles of their own — a tree over BSPNode is an HprtBspPaper, a tree over BSPKdNode an HprtBspPaperKd ----
int hprt_bspnode_build(const HprtModel *m, const HprtBspNodeParams *params, HprtBspPaper **out) try {
    return BuildBspNodeFromModel("hprt_bspnode_build", m, params, out);
} catch (...) { return hprt::HandleException(); }
int hprt_bspnode_build_from_triangles(size_t n, const float *p9, const HprtBspNodeParams *params, HprtBspPaper **out) try {
    return BuildBspNodeFromTriangles("hprt_bspnode_build_from_triangles", n, p9, params, out);
} catch (...) { return hprt::HandleException(); }
int hprt_bspnodekd_build(const HprtModel *m, const HprtBspNodeParams *params, HprtBspPaperKd **out) try {
    return BuildBspNodeFromModel("hprt_bspnodekd_build", m, params, out);
} catch (...) { return hprt::HandleException(); }
int hprt_bspnodekd_build_from_triangles(size_t n, const float *p9, const HprtBspNodeParams *params, HprtBspPaperKd **out) try {
    return BuildBspNodeFromTriangles("hprt_bspnodekd_build_from_triangles", n, p9, params, out);
} catch (...) { return hprt::HandleException(); }
// ---- the device-assisted builds: the same builder with its candidates costed by k_sweepcost (device/bspnode_cost.hip) ----
int hprt_bspnode_build_device(const HprtModel *m, const HprtBspNodeParams *params, const HprtBspBuildDeviceOpts *opts, HprtBuildDeviceStats *stats,
                              HprtBspPaper **out) try {
    BspNodeHook h; h.device = true; h.opts = opts; h.stats = stats;
    return BuildBspNodeFromModel("hprt_bspnode_build_device", m, params, out, &h);
} catch (...) { return hprt::HandleException(); }
int hprt_bspnode_build_from_triangles_device(size_t n, const float *p9, const HprtBspNodeParams *params, const HprtBspBuildDeviceOpts *opts,
                                             HprtBuildDeviceStats *stats, HprtBspPaper **out) try {
    BspNodeHook h; h.device = true; h.opts = opts; h.stats = stats;
    return BuildBspNodeFromTriangles("hprt_bspnode_build_from_triangles_device", n, p9, params, out, &h);
} catch (...) { return hprt::HandleException(); }
int hprt_bspnodekd_build_device(const HprtModel *m, const HprtBspNodeParams *params, const HprtBspBuildDeviceOpts *opts, HprtBuildDeviceStats *stats,
                                HprtBspPaperKd **out) try {
    BspNodeHook h; h.device = true; h.opts = opts; h.stats = stats;
    return BuildBspNodeFromModel("hprt_bspnodekd_build_device", m, params, out, &h);
} catch (...) { return hprt::HandleException(); }
int hprt_bspnodekd_build_from_triangles_device(size_t n, const float *p9, const HprtBspNodeParams *params, const HprtBspBuildDeviceOpts *opts,
                                               HprtBuildDeviceStats *stats, HprtBspPaperKd **out) try {
    BspNodeHook h; h.device = true; h.opts = opts; h.stats = stats;
    return BuildBspNodeFromTriangles("hprt_bspnodekd_build_from_triangles_device", n, p9, params, out, &h);
} catch (...) { return hprt::HandleException(); }
// ---- two-level node-based BSP trees (the nine names over object instances, core/api.cpp:1794-1819; BuildBspNodeInst above): the
// handle is HprtBspPaperInst, kd-aware for the fastkd form, and hprt_bsppaperinst_* / hprt_scene_attach_bsppaperinst serve it ----
int hprt_bspnodeinst_build(const HprtModel *m, const HprtBspNodeParams *params, HprtBspPaperInst **out) try {
    return BuildBspNodeInst("hprt_bspnodeinst_build", m, params, out);
} catch (...) { return hprt::HandleException(); }
int hprt_bspnodeinst_build_device(const HprtModel *m, const HprtBspNodeParams *params, const HprtBspBuildDeviceOpts *opts, HprtBuildDeviceStats *stats,
                                  HprtBspPaperInst **out) try {
    BspNodeHook h; h.device = true; h.opts = opts; h.stats = stats;
    return BuildBspNodeInst("hprt_bspnodeinst_build_device", m, params, out, &h);
} catch (...) { return hprt::HandleException(); }
// Diagnostics hooks of the node-based candidate costing (not part of include/hprt.h; tests/bspnode_cost_nodes.py).
// hprt_debug_bspnode_root_nodes hands out the first max_nodes nodes a build costs, in build order: mesh, the node's directions, the
// sweep's directions and the candidates, with the costs the builder's own code gave them.  m != NULL: the model's primitives; else n
// triangles.  The form in params selects the handle.  The pointers are valid during the call only.
__attribute__((visibility("default"))) int hprt_debug_bspnode_root_nodes(const HprtModel *m, size_t n, const float *p9, const HprtBspNodeParams *params,
                                                                          uint32_t max_nodes, BspSweepNodeSink sink, void *user) try {
    if (!params || !sink) return SetError(HPRT_E_INVALID, "hprt_debug_bspnode_root_nodes: null argument");
    BspNodeHook h; h.sink = sink; h.user = user; h.maxNodes = max_nodes;
    const char *fn = "hprt_debug_bspnode_root_nodes";
    int rc;
    if (params->form == BSPNODE_FASTKD) {
        HprtBspPaperKd *t = nullptr;
        rc = m ? BuildBspNodeFromModel(fn, m, params, &t, &h) : BuildBspNodeFromTriangles(fn, n, p9, params, &t, &h);
        delete t;
    } else {
        HprtBspPaper *t = nullptr;
        rc = m ? BuildBspNodeFromModel(fn, m, params, &t, &h) : BuildBspNodeFromTriangles(fn, n, p9, params, &t, &h);
        delete t;
    }
    return rc;
} catch (...) { return hprt::HandleException(); }
// hprt_debug_bspnode_cost costs a node again with impl 0 (the vector code of bsp_build.h, BspNodeCostVector), 1 (bspnode_cost.h on
// the host) or 2 (k_sweepcost).  nd: a node as the sink above receives it (costs / costs_fixed are not read; the scalars' capacity
// fields may lower the compiled capacities).  Everything the costing indexes by is checked first (HPRT_E_INVALID): M, every face id,
// every direction's kind against fastkd, every candidate's direction, the capacities.  *declined is 1 when impl 1 / 2 decline
// the node whole (its own mesh, faces, direction list or sweep beyond a capacity); every candidate then comes back flagged.
__attribute__((visibility("default"))) int hprt_debug_bspnode_cost(const HprtDebugBspSweepNode *nd, int fastkd, int impl, float *costs, float *costs_fixed,
                                                                    uint8_t *overflow, int *declined) try {
    using namespace bspnodecost;
    const char *fn = "hprt_debug_bspnode_cost: ";
    if (!nd || !costs || !costs_fixed || !overflow || !declined || !nd->scalars || !nd->dirs || !nd->sweep || (nd->n && !nd->cands) || (nd->n_edges && !nd->edges))
        return SetError(HPRT_E_INVALID, std::string(fn) + "null argument");
    if (impl < 0 || impl > 2) return SetError(HPRT_E_INVALID, std::string(fn) + "impl is not 0, 1 or 2");
    if (nd->M == 0 || nd->M > 65536u || nd->n_edges > 65536u || nd->n > 0x7fffffffull || nd->n_dirs == 0 || nd->n_dirs > 4096u)
        return SetError(HPRT_E_INVALID, std::string(fn) + "a size that cannot be real");
    Scalars sc;
    memcpy(&sc, nd->scalars, sizeof(sc));
    uint32_t cap[4];
    if (!bspcost::Capacities(sc, cap)) return SetError(HPRT_E_INVALID, std::string(fn) + "a capacity field may only lower the compiled capacity");
    std::vector<Edge> mesh(nd->n_edges);
    if (nd->n_edges) memcpy(static_cast<void *>(mesh.data()), nd->edges, (size_t)nd->n_edges * sizeof(Edge));
    for (const Edge &e : mesh)
        if (e.f1 >= 2 * nd->M || e.f2 >= 2 * nd->M) return SetError(HPRT_E_INVALID, std::string(fn) + "a face id is not below 2 M");
    std::vector<SweepDir> sweep(nd->n_dirs);
    memcpy(static_cast<void *>(sweep.data()), nd->sweep, (size_t)nd->n_dirs * sizeof(SweepDir));
    for (const SweepDir &sd : sweep)
        if (fastkd ? (sd.kind != KIND_KD_AXIS && sd.kind != KIND_CHOSEN) : sd.kind != KIND_PLAIN)
            return SetError(HPRT_E_INVALID, std::string(fn) + "a direction's kind is not one of the tree form's");
    std::vector<Cand> cs(nd->n);
    if (nd->n) memcpy(static_cast<void *>(cs.data()), nd->cands, nd->n * sizeof(Cand));
    for (const Cand &c : cs)
        if (c.k >= nd->n_dirs) return SetError(HPRT_E_INVALID, std::string(fn) + "a candidate's direction is not one of the sweep's");
    for (size_t k = 0; k < nd->n; ++k) { costs[k] = 0; costs_fixed[k] = std::numeric_limits<float>::infinity(); overflow[k] = 1; }
    *declined = 0;
    const BspNodeCostRequest rq{mesh.data(), nd->n_edges, nd->dirs, nd->M, sweep.data(), nd->n_dirs, fastkd != 0, sc, cs.data(), nd->n, costs,
                                fastkd ? costs_fixed : nullptr, overflow, 0u};
    int rc = 0;
    if (impl == 0) BspNodeCostVector(rq);
    else if (impl == 1) rc = BspNodeCostRestated(rq);
    else {
        std::string err;
        const uint32_t asked[3] = {sc.maxEdges, sc.maxFaces, sc.maxFaceEdges};
        BspNodeCostDevice *d = nullptr;
        int drc = BspNodeCostDeviceCreate(0, asked, &d, &err);
        const BspNodeDevicePtr dev(d);
        if (drc != HPRT_OK) return SetError(drc, err);
        rc = BspNodeCostOnDevice(d, cap, rq, &drc, &err);
        if (rc < 0) return SetError(drc, err);
    }
    if (rc == 1) { *declined = 1; return HPRT_OK; }
    for (size_t k = 0; k < nd->n; ++k)
        if (overflow[k]) { costs[k] = 0; costs_fixed[k] = std::numeric_limits<float>::infinity(); }
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
// Diagnostics hooks (not part of include/hprt.h; tests/test_bspnode_host.py).  hprt_debug_bspnode_choose: `draws` calls of a
// direction chooser over the triangles p9 from one engine seeded with `seed`; counts[k] = directions of call k, dirs their
// components in order (room for draws * max(K, n) * 3 floats).  hprt_debug_bspnode_check: the structural check of a tree given as
// 20-byte nodes (kd_aware: BSPKdNode's flags), its depth in *depth; returns HPRT_E_UNSUPPORTED past the walks' 64 levels.
__attribute__((visibility("default"))) int hprt_debug_bspnode_choose(int chooser, uint32_t K, uint32_t seed, size_t n, const float *p9, uint32_t draws,
                                                                      uint32_t *counts, float *dirs) try {
    std::vector<uint32_t> c; std::vector<float> d;
    const std::string err = BspNodeChoose(chooser, K, seed, n, p9, draws, &c, &d);
    if (!err.empty()) return SetError(HPRT_E_UNSUPPORTED, err);
    std::copy(c.begin(), c.end(), counts);
    std::copy(d.begin(), d.end(), dirs);
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
__attribute__((visibility("default"))) int hprt_debug_bspnode_check(size_t n_nodes, const uint32_t *nodes20, size_t n_idx, const uint32_t *idx, uint32_t n_prims,
                                                                     int kd_aware, uint32_t *depth) try {
    BspPaperTree t;
    t.kdAware = kd_aware != 0; t.nPrims = n_prims;
    for (size_t k = 0; k < n_nodes; ++k) {
        t.nodes.push_back(BspNode{nodes20[5 * k], nodes20[5 * k + 1]});
        float a[3]; memcpy(a, &nodes20[5 * k + 2], 12);
        t.axes.insert(t.axes.end(), a, a + 3);
    }
    t.primIndices.assign(idx, idx + n_idx);
    const char *bad = t.kdAware ? CheckBspPaperKdTree(t, depth) : CheckBspPaperTree(t, depth);
    if (*bad) return SetError(HPRT_E_INVALID, std::string("malformed tree: ") + bad);
    if (*depth > BspPaperTodoMax(t.kdAware)) return SetError(HPRT_E_UNSUPPORTED, TooDeepMessage("node-based BSP tree", *depth));
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
// Diagnostics hooks (not part of include/hprt.h; tests/deep_todo.py): a tree made by hand as an ordinary handle, so that a tree with a
// known todo depth reaches the walks.  nodes8 / nodes20: the node words as hprt_<tree>_copy writes them; idx: primitiveIndices; n_prims:
// the primitives the tree is over (creation-order numbers); bounds6: the tree's bounds, pMin then pMax; M: the direction set of the
// library's own table.  The tree passes the structural check and the depth limit a built tree passes (HPRT_E_INVALID,
// HPRT_E_UNSUPPORTED), and hprt_scene_attach_* checks it again like any other.
__attribute__((visibility("default"))) int hprt_debug_kdtree_from_arrays(size_t n_nodes, const uint32_t *nodes8, size_t n_idx, const uint32_t *idx, uint32_t n_prims,
                                                                          const float *bounds6, HprtKdTree **out) try {
    if (!out || !nodes8 || !bounds6 || (n_idx && !idx)) return SetError(HPRT_E_INVALID, "hprt_debug_kdtree_from_arrays: null argument");
    std::unique_ptr<HprtKdTree> t(new HprtKdTree());
    KdTree &k = t->tree;
    k.nPrims = n_prims;
    k.nodes.resize(n_nodes);
    memcpy(k.nodes.data(), nodes8, n_nodes * sizeof(KdNode));
    k.primIndices.assign(idx, idx + n_idx);
    memcpy(k.bounds, bounds6, sizeof(k.bounds));
    const char *bad = CheckKdTree(k, &k.depth);
    if (*bad) return SetError(HPRT_E_INVALID, std::string("malformed tree: ") + bad);
    k.maxDepth = k.depth; k.leaves = CountLeaves(k.nodes, 3u, 3u);
    return FinishKdTree(t.release(), out);
} catch (...) { return hprt::HandleException(); }
// Diagnostics hooks of the candidate costing (tests/test_kdop_cost_host.py, tests/test_gpu_kdop_cost.py).
// hprt_debug_kdop_cost costs a caller's mesh and candidates with impl 0 (the vector code of kdop_mesh.h, RbspCostVector), 1
// (kdop_cost.h on the host) or 2 (k_kdopcost).  edges: n_edges records of 32 bytes (v1, v2, f1, f2); scalars: kdopcost::Scalars (7
// words: invTotalSA, emptyBonus, isectCost, traversalCost, kdTraversalCost, nPrimitives, maxEdges); cands: n records of 20 bytes
// (d, i, nBelow, nAbove, t).  Everything the costing indexes by is checked first: M, n_edges, every face id, every candidate's d,
// maxEdges (HPRT_E_INVALID).  A mesh of more edges than maxEdges allows is not costed by impl 1 / 2: every candidate is flagged.
__attribute__((visibility("default"))) int hprt_debug_kdop_cost(const void *edges, uint32_t n_edges, uint32_t M, int kd_aware, const void *scalars,
                                                                 const void *cands, size_t n, int impl, float *costs, float *costs_fixed,
                                                                 uint8_t *overflow) try {
    using namespace kdopcost;
    if (!scalars || !costs || !costs_fixed || !overflow || (n && !cands) || (n_edges && !edges))
        return SetError(HPRT_E_INVALID, "hprt_debug_kdop_cost: null argument");
    if (M != 3 && M != 7 && M != 9 && M != 13) return SetError(HPRT_E_INVALID, "hprt_debug_kdop_cost: M is not 3, 7, 9 or 13");
    if (impl < 0 || impl > 2) return SetError(HPRT_E_INVALID, "hprt_debug_kdop_cost: impl is not 0, 1 or 2");
    if (n_edges > 65536u || n > 0xffffffffull) return SetError(HPRT_E_INVALID, "hprt_debug_kdop_cost: a size that cannot be real");
    Scalars sc;
    memcpy(&sc, scalars, sizeof(sc));
    if (sc.maxEdges > KDOP_MAX_EDGES) return SetError(HPRT_E_INVALID, "hprt_debug_kdop_cost: maxEdges may only lower the compiled capacity");
    const uint32_t cap = sc.maxEdges ? sc.maxEdges : (uint32_t)KDOP_MAX_EDGES;
    std::vector<Edge> mesh(n_edges);
    if (n_edges) memcpy(static_cast<void *>(mesh.data()), edges, (size_t)n_edges * sizeof(Edge));
    for (const Edge &e : mesh)
        if (e.f1 >= 2 * M || e.f2 >= 2 * M) return SetError(HPRT_E_INVALID, "hprt_debug_kdop_cost: a face id is not below 2 M");
    std::vector<Cand> cs(n);
    if (n) memcpy(static_cast<void *>(cs.data()), cands, n * sizeof(Cand));
    for (const Cand &c : cs)
        if (c.d >= M) return SetError(HPRT_E_INVALID, "hprt_debug_kdop_cost: a candidate's direction is not below M");
    std::vector<float> dirs;
    RbspDirections(M, &dirs);
    for (size_t k = 0; k < n; ++k) { costs[k] = 0; costs_fixed[k] = 0; overflow[k] = 1; }
    if (impl == 0) {
        RbspCostRequest rq{mesh.data(), n_edges, dirs.data(), M, kd_aware != 0, sc, cs.data(), n, costs, costs_fixed, overflow};
        RbspCostVector(rq);
        return HPRT_OK;
    }
    if (n_edges > cap) return HPRT_OK;      // every candidate flagged
    if (impl == 1) {
        std::vector<Q> words(kStoreWords);
        uint8_t list[KDOP_MAX_FACE_EDGES];
        Store st;
        st.left = words.data(); st.right = words.data() + 2 * KDOP_MAX_EDGES; st.fv = words.data() + 4 * KDOP_MAX_EDGES; st.stride = 1;
        st.flist = list; st.fstride = 1; st.cap = cap;
        for (size_t k = 0; k < n; ++k) CostCandidate(mesh.data(), n_edges, dirs.data(), M, kd_aware != 0, sc, cs[k], st, &costs[k], &costs_fixed[k], &overflow[k]);
        return HPRT_OK;
    }
    std::string err;
    KdopCostDevice *d = nullptr;
    int rc = KdopCostDeviceCreate(0, sc.maxEdges, &d, &err);
    const KdopDevicePtr dev(d);
    if (rc != HPRT_OK) return SetError(rc, err);
    rc = KdopCostDeviceRun(d, mesh.data(), n_edges, dirs.data(), M, kd_aware != 0, sc, cs.data(), n, costs, costs_fixed, overflow, &err);
    if (rc != HPRT_OK) return SetError(rc, err);
    if (!kd_aware) for (size_t k = 0; k < n; ++k) costs_fixed[k] = 0;
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
// The mesh, the scalars and the candidates of the first max_nodes nodes a build costs, in build order, each with the costs the
// builder's own code (costRange) gave them; the meshes are the builder's, reoriented as its SurfaceArea calls left them.  m != NULL:
// the model's primitives (hprt_rbsp_build / hprt_rbspkd_build); else n triangles.  params: HprtRbspKdParams for both trees
// (kd_trav_cost is not read when kd_aware is 0).  sink(user, node, edges, n_edges, scalars, cands, n, costs, costs_fixed):
// costs_fixed is NULL unless kd_aware; the pointers are valid during the call only.
__attribute__((visibility("default"))) int hprt_debug_rbsp_root_mesh(const HprtModel *m, size_t n, const float *p9, int kd_aware, const HprtRbspKdParams *params,
                                                                      uint32_t max_nodes, RbspNodeSink sink, void *user) try {
    if (!params || !sink) return SetError(HPRT_E_INVALID, "hprt_debug_rbsp_root_mesh: null argument");
    RbspHook h; h.sink = sink; h.user = user; h.maxNodes = max_nodes;
    int rc;
    if (kd_aware) {
        HprtRbspKd *t = nullptr;
        rc = m ? BuildRbspFromModel("hprt_debug_rbsp_root_mesh", "rbspkd", m, params, RbspParams(), &t, &h)
               : BuildRbspFromTriangles("hprt_debug_rbsp_root_mesh", n, p9, params, &t, &h);
        delete t;
    } else {
        const HprtRbspParams q{params->isect_cost, params->trav_cost, params->empty_bonus, params->max_prims, params->max_depth, params->n_directions, params->threads};
        HprtRbsp *t = nullptr;
        rc = m ? BuildRbspFromModel("hprt_debug_rbsp_root_mesh", "RBSP", m, &q, RbspParams(), &t, &h)
               : BuildRbspFromTriangles("hprt_debug_rbsp_root_mesh", n, p9, &q, &t, &h);
        delete t;
    }
    return rc;
} catch (...) { return hprt::HandleException(); }
__attribute__((visibility("default"))) int hprt_debug_rbsp_from_arrays(uint32_t M, size_t n_nodes, const uint32_t *nodes8, size_t n_idx, const uint32_t *idx,
                                                                        uint32_t n_prims, const float *bounds6, HprtRbsp **out) try {
    return RbspFromArrays("hprt_debug_rbsp_from_arrays", M, n_nodes, nodes8, n_idx, idx, n_prims, bounds6, out);
} catch (...) { return hprt::HandleException(); }
__attribute__((visibility("default"))) int hprt_debug_rbspkd_from_arrays(uint32_t M, size_t n_nodes, const uint32_t *nodes8, size_t n_idx, const uint32_t *idx,
                                                                          uint32_t n_prims, const float *bounds6, HprtRbspKd **out) try {
    return RbspFromArrays("hprt_debug_rbspkd_from_arrays", M, n_nodes, nodes8, n_idx, idx, n_prims, bounds6, out);
} catch (...) { return hprt::HandleException(); }
__attribute__((visibility("default"))) int hprt_debug_bsppaper_from_arrays(size_t n_nodes, const uint32_t *nodes20, size_t n_idx, const uint32_t *idx, uint32_t n_prims,
                                                                            const float *bounds6, HprtBspPaper **out) try {
    return BspPaperFromArrays("hprt_debug_bsppaper_from_arrays", n_nodes, nodes20, n_idx, idx, n_prims, bounds6, out);
} catch (...) { return hprt::HandleException(); }
__attribute__((visibility("default"))) int hprt_debug_bsppaperkd_from_arrays(size_t n_nodes, const uint32_t *nodes20, size_t n_idx, const uint32_t *idx, uint32_t n_prims,
                                                                              const float *bounds6, HprtBspPaperKd **out) try {
    return BspPaperFromArrays("hprt_debug_bsppaperkd_from_arrays", n_nodes, nodes20, n_idx, idx, n_prims, bounds6, out);
} catch (...) { return hprt::HandleException(); }
// Diagnostics hooks (not part of include/hprt.h; tests/test_bsppaper_host.py), the bsppaper builder's views of the triangles p9
// (9 floats each, creation order).  hprt_debug_bsppaper_planes: getBSPPaperPlanes of triangle 0, planes_out[4 k ..] = {t, axis}
// of its k-th plane (room for 4); returns how many in *n_planes.
__attribute__((visibility("default"))) int hprt_debug_bsppaper_planes(const float *p9, float *planes_out, uint32_t *n_planes) try {
    if (!p9 || !planes_out || !n_planes) return SetError(HPRT_E_INVALID, "hprt_debug_bsppaper_planes: null argument");
    const std::vector<BspPlane> pl = BspPaperTrianglePlanes(p9);
    *n_planes = (uint32_t)pl.size();
    for (size_t k = 0; k < pl.size(); ++k) memcpy(planes_out + 4 * k, &pl[k], 16);
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
// hprt_debug_bsppaper_classify: the plane plane4 = {t, axis} over a BVH of the n triangles (isectCost 4, travCost 8, maxPrims 1):
// counts[2] from getAmountToLeftAndRight, and the left / right lists of getPrimnumsToLeftAndRight (local numbers, up to cap
// entries each; sizes[2] their full lengths).
__attribute__((visibility("default"))) int hprt_debug_bsppaper_classify(size_t n, const float *p9, const float *plane4, uint32_t counts[2],
                                                                        uint32_t *left, uint32_t *right, size_t cap, uint32_t sizes[2]) try {
    if (n == 0 || !p9 || !plane4 || !counts || !left || !right || !sizes) return SetError(HPRT_E_INVALID, "hprt_debug_bsppaper_classify: bad argument");
    std::vector<float> lo, hi;
    RbspTriangleBounds(n, p9, &lo, &hi);
    std::vector<uint8_t> isTri(n, 1);
    BspPlane plane;
    memcpy(&plane, plane4, 16);
    std::vector<uint32_t> l, r;
    BspPaperClassify(n, lo.data(), hi.data(), p9, isTri.data(), plane, counts, &l, &r);
    sizes[0] = (uint32_t)l.size(); sizes[1] = (uint32_t)r.size();
    for (size_t k = 0; k < l.size() && k < cap; ++k) left[k] = l[k];
    for (size_t k = 0; k < r.size() && k < cap; ++k) right[k] = r[k];
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
int hprt_bvh_info(const HprtBvh *b, uint32_t info[4], float bounds6[6]) try {
    if (!b || !info) return SetError(HPRT_E_INVALID, "hprt_bvh_info: null argument");
    info[0] = (uint32_t)b->tree.nodes.size(); info[1] = (uint32_t)b->tree.primOrder.size();
    info[2] = (uint32_t)b->tree.nLeaves; info[3] = (uint32_t)b->tree.maxDepth;
    if (bounds6) {
        if (b->tree.nodes.empty()) for (int i = 0; i < 6; ++i) bounds6[i] = 0;
        else { memcpy(bounds6, b->tree.nodes[0].bmin, 12); memcpy(bounds6 + 3, b->tree.nodes[0].bmax, 12); }
    }
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
int hprt_bvh_copy(const HprtBvh *b, void *nodes32, uint32_t *prim_order) try {
    if (!b) return SetError(HPRT_E_INVALID, "hprt_bvh_copy: null argument");
    if (nodes32 && !b->tree.nodes.empty()) memcpy(nodes32, b->tree.nodes.data(), b->tree.nodes.size() * sizeof(BvhNode));
    if (prim_order && !b->tree.primOrder.empty()) memcpy(prim_order, b->tree.primOrder.data(), b->tree.primOrder.size() * 4);
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }

int hprt_bvh_object_info(const HprtBvh *b, uint32_t object, uint32_t info[4], float bounds6[6]) try {
    if (!b || !info || object >= b->objects.size()) return SetError(HPRT_E_INVALID, "hprt_bvh_object_info: bad argument");
    const BvhTree &t = b->objects[object];
    info[0] = (uint32_t)t.nodes.size(); info[1] = (uint32_t)t.primOrder.size(); info[2] = (uint32_t)t.nLeaves; info[3] = (uint32_t)t.maxDepth;
    if (bounds6) {
        if (t.nodes.empty()) for (int i = 0; i < 6; ++i) bounds6[i] = 0;
        else { memcpy(bounds6, t.nodes[0].bmin, 12); memcpy(bounds6 + 3, t.nodes[0].bmax, 12); }
    }
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }
int hprt_bvh_object_copy(const HprtBvh *b, uint32_t object, void *nodes32, uint32_t *prim_order) try {
    if (!b || object >= b->objects.size()) return SetError(HPRT_E_INVALID, "hprt_bvh_object_copy: bad argument");
    const BvhTree &t = b->objects[object];
    if (nodes32 && !t.nodes.empty()) memcpy(nodes32, t.nodes.data(), t.nodes.size() * sizeof(BvhNode));
    if (prim_order && !t.primOrder.empty()) memcpy(prim_order, t.primOrder.data(), t.primOrder.size() * 4);
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }

int hprt_halton_permutations(uint16_t *out, size_t max_entries, size_t *n_entries) try {
    const std::vector<uint16_t> &p = HaltonPermutations();
    if (n_entries) *n_entries = p.size();
    if (out) memcpy(out, p.data(), 2 * (p.size() < max_entries ? p.size() : max_entries));
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }

}  // extern "C"
// The records of a parsed model and its BVH as an HprtSceneDesc of borrowed pointers, handed to `use`
template <class Use>
static int WithModelDesc(const HprtModel *m, const HprtBvh *b, Use use) {
    const SceneModel &sm = m->sc;
    std::vector<HprtShapeDesc> shapes(sm.shapes.size());
    for (size_t i = 0; i < sm.shapes.size(); ++i) {
        const ShapeDesc &s = sm.shapes[i];
        HprtShapeDesc &o = shapes[i];
        memset(&o, 0, sizeof(o));
        o.kind = s.kind; o.material = s.material; o.area_light = s.areaLight;
        o.reverse_orientation = s.reverseOrientation; o.transform_swaps_handedness = s.transformSwapsHandedness;
        if (s.kind == kTriangleMesh) {
            o.n_tris = s.mesh.nTris(); o.n_verts = s.mesh.nVerts();
            o.indices = s.mesh.indices.data(); o.P = s.mesh.P.data();
            o.N = s.mesh.N.empty() ? nullptr : s.mesh.N.data();
            o.UV = s.mesh.UV.empty() ? nullptr : s.mesh.UV.data();
            o.S = s.mesh.S.empty() ? nullptr : s.mesh.S.data();
        } else {
            memcpy(o.object_to_world, s.sphere.objectToWorld.m, 64); memcpy(o.world_to_object, s.sphere.worldToObject.m, 64);
            o.radius = s.sphere.radius; o.z_min = s.sphere.zMin; o.z_max = s.sphere.zMax;
            o.theta_min = s.sphere.thetaMin; o.theta_max = s.sphere.thetaMax; o.phi_max = s.sphere.phiMax;
        }
    }
    std::vector<HprtMaterialDesc> mats(sm.materials.size());
    for (size_t i = 0; i < mats.size(); ++i) {
        const MaterialDesc &s = sm.materials[i];
        mats[i].type = s.type; memcpy(mats[i].Kd, s.Kd, 12); mats[i].sigma = s.sigma; memcpy(mats[i].Ks, s.Ks, 12);
        mats[i].roughness = s.roughness; mats[i].remap_roughness = s.remapRoughness;
        mats[i].kd_texture = s.KdTex; mats[i].ks_texture = s.KsTex; mats[i].opacity_texture = s.opacityTex;
        memcpy(mats[i].Kr, s.Kr, 12); memcpy(mats[i].Kt, s.Kt, 12); memcpy(mats[i].opacity, s.opacity, 12); mats[i].eta = s.eta;
    }
    std::vector<std::vector<HprtTextureLevel>> texLevels(sm.textures.size());
    std::vector<HprtTextureDesc> textures(sm.textures.size());
    for (size_t i = 0; i < textures.size(); ++i) {
        const TextureDesc &t = sm.textures[i];
        for (const MipLevel &l : t.levels) texLevels[i].push_back(HprtTextureLevel{l.w, l.h, l.rgb.data()});
        textures[i].levels = texLevels[i].data(); textures[i].n_levels = (uint32_t)texLevels[i].size();
        textures[i].trilinear = t.trilinear; textures[i].max_anisotropy = t.maxAniso; textures[i].wrap = t.wrap;
        textures[i].su = t.su; textures[i].sv = t.sv; textures[i].du = t.du; textures[i].dv = t.dv; textures[i].weight_lut = t.weightLut;
    }
    std::vector<HprtLightDesc> lights(sm.lights.size());
    for (size_t i = 0; i < lights.size(); ++i) {
        const LightDesc &s = sm.lights[i];
        lights[i].type = s.type; memcpy(lights[i].pos, s.pos, 12); memcpy(lights[i].I, s.I, 12); lights[i].shape = s.shape; lights[i].two_sided = s.twoSided;
        lights[i].texture = s.texture; memcpy(lights[i].light_to_world, &s.lightToWorld, 64); memcpy(lights[i].world_to_light, &s.worldToLight, 64);
    }
    if (b->objects.size() != sm.nObjects) return SetError(HPRT_E_INVALID, "the BVH was built for another model (object count differs)");
    // object definitions: their shapes are contiguous (no nesting of definitions, core/api.cpp:1755-1756)
    std::vector<HprtObjectDesc> objects(sm.nObjects);
    for (uint32_t k = 0; k < sm.nObjects; ++k) {
        HprtObjectDesc &o = objects[k];
        memset(&o, 0, sizeof(o));
        bool any = false;
        for (size_t i = 0; i < sm.shapes.size(); ++i)
            if (sm.shapes[i].object == (int32_t)k) { if (!any) { o.first_shape = (uint32_t)i; any = true; } o.n_shapes = (uint32_t)i + 1u - o.first_shape; }
        const BvhTree &t = b->objects[k];
        o.nodes = t.nodes.data(); o.n_nodes = (uint32_t)t.nodes.size(); o.prim_order = t.primOrder.data(); o.n_prims = (uint32_t)t.primOrder.size();
    }
    std::vector<HprtInstanceDesc> instances(sm.instances.size());
    for (size_t i = 0; i < instances.size(); ++i) {
        instances[i].object = sm.instances[i].object;
        memcpy(instances[i].instance_to_world, sm.instances[i].instanceToWorld.m, 64);
        memcpy(instances[i].world_to_instance, sm.instances[i].worldToInstance.m, 64);
    }
    std::vector<HprtTopItem> top(sm.top.size());
    for (size_t i = 0; i < top.size(); ++i) { top[i].kind = sm.top[i].kind; top[i].index = sm.top[i].index; }
    HprtSceneDesc d;
    memset(&d, 0, sizeof(d));
    d.textures = textures.data(); d.n_textures = (uint32_t)textures.size();
    d.objects = objects.data(); d.n_objects = (uint32_t)objects.size();
    d.instances = instances.data(); d.n_instances = (uint32_t)instances.size();
    static const HprtTopItem kNoItems[1] = {{0, 0u}};
    d.top = top.empty() ? kNoItems : top.data(); d.n_top = (uint32_t)top.size();
    d.nodes = b->tree.nodes.data(); d.n_nodes = (uint32_t)b->tree.nodes.size();
    d.prim_order = b->tree.primOrder.data(); d.n_prims = (uint32_t)b->tree.primOrder.size();
    d.shapes = shapes.data(); d.n_shapes = (uint32_t)shapes.size();
    d.materials = mats.data(); d.n_materials = (uint32_t)mats.size();
    d.lights = lights.data(); d.n_lights = (uint32_t)lights.size();
    // a single light always gets the uniform distribution (core/lightdistrib.cpp:50-52)
    d.light_strategy = sm.lights.size() <= 1 ? 0 : sm.opt.lightStrategy;
    return use(d);
}
extern "C" {
// hprt_scene_create over a parsed model and its BVH
int hprt_scene_create_from_model(const HprtModel *m, const HprtBvh *b, int device, HprtScene **out) try {
    if (!m || !b || !out) return SetError(HPRT_E_INVALID, "hprt_scene_create_from_model: null argument");
    return WithModelDesc(m, b, [&](const HprtSceneDesc &d) { return hprt_scene_create(&d, device, out); });
} catch (...) { return hprt::HandleException(); }
// Diagnostics hook (not part of include/hprt.h; tests/test_distant_grid_host.py): the host half of hprt_scene_create_from_model, no
// device — which shadow grid the scene's layout holds.  out8 = {point grid: eligible, R; distant grid: eligible, R, entries, near-list
// length, bytes of the image, longest list}
__attribute__((visibility("default"))) int hprt_debug_shadow_grid_layout(const HprtModel *m, const HprtBvh *b, double out8[8]) try {
    if (!m || !b || !out8) return SetError(HPRT_E_INVALID, "hprt_debug_shadow_grid_layout: null argument");
    return WithModelDesc(m, b, [&](const HprtSceneDesc &d) { return LayoutGridsForDebug(d, out8); });
} catch (...) { return hprt::HandleException(); }

// Film::WriteImage, core/film.cpp:266-303 (no splats)
int hprt_film_resolve(const float *xyzw, size_t n, float scale, float *rgb) try {
    if (!xyzw || !rgb) return SetError(HPRT_E_INVALID, "hprt_film_resolve: null argument");
    for (size_t i = 0; i < n; ++i) {
        const float *x = &xyzw[4 * i];
        float *o = &rgb[3 * i];
        o[0] = 3.240479f * x[0] - 1.537150f * x[1] - 0.498535f * x[2];
        o[1] = -0.969256f * x[0] + 1.875991f * x[1] + 0.041556f * x[2];
        o[2] = 0.055648f * x[0] - 0.204043f * x[1] + 1.057311f * x[2];
        float w = x[3];
        if (w != 0) {
            float invWt = 1.0f / w;
            o[0] = sel_max(0.f, o[0] * invWt); o[1] = sel_max(0.f, o[1] * invWt); o[2] = sel_max(0.f, o[2] * invWt);
        }
        // splat term: XYZToRGB(0) = +0 in every channel; v + 1*0 keeps v (and turns -0 into +0)
        o[0] += 0.f; o[1] += 0.f; o[2] += 0.f;
        o[0] *= scale; o[1] *= scale; o[2] *= scale;
    }
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }

int hprt_write_pixel_stats(const char *prefix, const uint64_t *stats7, int width, int height) try {
    return hprt_write_pixel_stats_accel(prefix, stats7, width, height, HPRT_ACCEL_BVH);
} catch (...) { return hprt::HandleException(); }
int hprt_write_pixel_stats_accel(const char *prefix, const uint64_t *stats7, int width, int height, int accel) try {
    if (!prefix || !stats7 || width <= 0 || height <= 0) return SetError(HPRT_E_INVALID, "hprt_write_pixel_stats: bad argument");
    if (accel != HPRT_ACCEL_BVH && accel != HPRT_ACCEL_KDTREE && accel != HPRT_ACCEL_RBSP) return SetError(HPRT_E_INVALID, "hprt_write_pixel_stats_accel: unknown accelerator");
    // per matrix, the index of its value in stats7 (-1: zero for this accelerator): a kd render's interior-node counts (slots 5, 6)
    // are its kdTreeNodeTraversals[P], an RBSP render's its bspTreeNodeTraversals[P]
    const int kd = accel == HPRT_ACCEL_KDTREE ? 5 : -1, kdP = accel == HPRT_ACCEL_KDTREE ? 6 : -1;
    const int bsp = accel == HPRT_ACCEL_RBSP ? 5 : -1, bspP = accel == HPRT_ACCEL_RBSP ? 6 : -1;
    const int field[8] = {1, 2, kd, kdP, bsp, bspP, 3, 4};
    return WriteStatMatrices(prefix, width, height, [&](int k, size_t i) { return field[k] < 0 ? 0ull : (unsigned long long)stats7[7 * i + field[k]]; });
} catch (...) { return hprt::HandleException(); }

// An rbspkd render's matrices: the kd share of slots 5 / 6 from kd2, the rest of them (oblique interior nodes) as bsp
int hprt_write_pixel_stats_rbspkd(const char *prefix, const uint64_t *stats7, const uint64_t *kd2, int width, int height) try {
    if (!prefix || !stats7 || !kd2 || width <= 0 || height <= 0) return SetError(HPRT_E_INVALID, "hprt_write_pixel_stats_rbspkd: bad argument");
    const size_t nPix = (size_t)width * (size_t)height;
    for (size_t i = 0; i < nPix; ++i)
        if (kd2[i] > stats7[7 * i + 5] || kd2[nPix + i] > stats7[7 * i + 6])
            return SetError(HPRT_E_INVALID, "hprt_write_pixel_stats_rbspkd: a pixel's kd share exceeds its interior-node count");
    // field: slot of stats7; kdPlane: the plane of kd2 that is the matrix (field -1) or is subtracted from the slot, -1 none
    const int field[8] = {1, 2, -1, -1, 5, 6, 3, 4}, kdPlane[8] = {-1, -1, 0, 1, 0, 1, -1, -1};
    return WriteStatMatrices(prefix, width, height, [&](int k, size_t i) {
        const unsigned long long kd = kdPlane[k] < 0 ? 0ull : (unsigned long long)kd2[(size_t)kdPlane[k] * nPix + i];
        return field[k] < 0 ? kd : (unsigned long long)stats7[7 * i + field[k]] - kd;
    });
} catch (...) { return hprt::HandleException(); }

// WritePFM, core/imageio.cpp:437+ : "PF", width height, scale -1 (little endian), rows bottom to top
int hprt_write_pfm(const char *path, const float *rgb, int width, int height) try {
    if (!path || !rgb || width <= 0 || height <= 0) return SetError(HPRT_E_INVALID, "hprt_write_pfm: bad argument");
    FILE *fp = fopen(path, "wb");
    if (!fp) return SetError(HPRT_E_IO, std::string("cannot create ") + path);
    bool ok = fprintf(fp, "PF\n%d %d\n-1.000000\n", width, height) > 0;
    for (int y = height - 1; y >= 0 && ok; --y) ok = fwrite(&rgb[3 * (size_t)y * width], sizeof(float), 3 * (size_t)width, fp) == 3 * (size_t)width;
    if (fclose(fp) != 0) ok = false;
    return ok ? HPRT_OK : SetError(HPRT_E_IO, std::string("write error on ") + path);
} catch (...) { return hprt::HandleException(); }

// Film::MergeFilmTile's accumulation (core/film.cpp:124-131) for cross-tile records on a host copy of the film: per
// destination pixel in ascending source-tile order, exactly as the single-GPU film kernels add them.
int hprt_film_records_merge(float *xyzw, size_t n_pixels, HprtFilmRecord *rec, size_t n) try {
    if (!xyzw || (n && !rec)) return SetError(HPRT_E_INVALID, "hprt_film_records_merge: null argument");
    std::sort(rec, rec + n, [](const HprtFilmRecord &a, const HprtFilmRecord &b) {
        return a.dest_pixel != b.dest_pixel ? a.dest_pixel < b.dest_pixel : a.src_tile < b.src_tile;
    });
    for (size_t i = 0; i < n; ++i) if (rec[i].dest_pixel >= n_pixels) return SetError(HPRT_E_INVALID, "film record outside the film");
    for (size_t i = 0; i < n; ++i) {
        float *px = xyzw + 4 * (size_t)rec[i].dest_pixel;
        px[0] += rec[i].xyz[0]; px[1] += rec[i].xyz[1]; px[2] += rec[i].xyz[2]; px[3] += rec[i].weight;
    }
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }

// Diagnostics hook (not part of include/hprt.h): the reference's unit tests for the host/device-shared math of this path,
// run over the product's own functions (hprt_math.h) on the host:
//   failures[0]  FloatingPoint.NextUpDownFloat   src/tests/fp_tests.cpp:29-47    next_up / next_down
//   failures[1]  Distribution1D.Discrete          src/tests/sampling.cpp:231-282  dist1d_build / dist1d_sample_discrete
__attribute__((visibility("default"))) int hprt_debug_host_selftest(int failures[2]) try {
    if (!failures) return HPRT_E_INVALID;
    const float inf = std::numeric_limits<float>::infinity();
    int f = 0;
    if (!(next_up(-0.f) > 0.f)) ++f;
    if (!(next_down(0.f) < 0.f)) ++f;
    if (!(next_up(inf) == inf)) ++f;
    if (!(next_down(inf) < inf)) ++f;
    if (!(next_down(-inf) == -inf)) ++f;
    if (!(next_up(-inf) > -inf)) ++f;
    // the default-seeded PCG32 stream of the reference's test (core/rng.h:61-62, 86-95)
    uint64_t state = 0x853c49e6748fea9bULL; const uint64_t inc = 0xda3e39cb94b95bdbULL;
    auto next32 = [&]() {
        uint64_t old = state;
        state = old * 0x5851f42d4c957f2dULL + inc;
        uint32_t xs = (uint32_t)(((old >> 18u) ^ old) >> 27u), rot = (uint32_t)(old >> 59u);
        return (xs >> rot) | (xs << ((~rot + 1u) & 31));
    };
    for (int i = 0; i < 100000; ++i) {
        float v;
        do { v = u2f(next32()); } while (std::isnan(v));
        if (std::isinf(v)) continue;
        if (std::nextafter(v, inf) != next_up(v)) ++f;
        if (std::nextafter(v, -inf) != next_down(v)) ++f;
    }
    failures[0] = f;
    f = 0;
    const float func[4] = {0, 1.f, 0.f, 3.f};
    float cdf[5], funcInt;
    dist1d_build(func, 4, cdf, &funcInt);
    float pdf;
    const float us[7] = {0.f, 0.125f, .24999f, .250001f, 0.625f, 0x1.fffffep-1f, 1.f};
    const int want[7] = {1, 1, 1, 3, 3, 3, 3};
    for (int k = 0; k < 7; ++k) {
        if (dist1d_sample_discrete(cdf, func, funcInt, 4, us[k], &pdf) != want[k]) ++f;
        if (pdf != (want[k] == 1 ? 0.25f : 0.75f)) ++f;
    }
    float u = .25f, uMax = .25f;
    for (int i = 0; i < 20; ++i) { u = next_down(u); uMax = next_up(uMax); }
    for (; u < uMax; u = next_up(u)) {
        int interval = dist1d_sample_discrete(cdf, func, funcInt, 4, u, &pdf);
        if (interval == 3) break;
        if (interval != 1) ++f;
    }
    if (!(u < uMax)) ++f;
    for (; u <= uMax; u = next_up(u))
        if (dist1d_sample_discrete(cdf, func, funcInt, 4, u, &pdf) != 3) ++f;
    failures[1] = f;
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }

// Diagnostics hook (not part of include/hprt.h; tests/test_wide_walk.py): the four-wide records BuildWide (wide_bvh.h) makes of a
// linear node array.  Every leaf gets the "boxed" reference ~firstPrimitive & ~WIDE_LEAF_BOXED (the single-triangle shortcut is
// decided at scene creation, where the vertices are).  out64: cap records of 64 bytes; *n_out: records made; *stack_need: the
// deepest stack a walk can hold.  HPRT_E_INVALID for a malformed array (CheckBvhNodes); HPRT_E_UNSUPPORTED when the tree keeps the
// binary walk (non-finite box, extent beyond the grid).
__attribute__((visibility("default"))) int hprt_debug_wide_build(const void *nodes32, uint32_t n_nodes, void *out64, size_t cap, size_t *n_out, int *stack_need) try {
    if (!nodes32 || !n_out || !stack_need) return SetError(HPRT_E_INVALID, "hprt_debug_wide_build: null argument");
    const BvhNode *nd = (const BvhNode *)nodes32;
    const char *bad = CheckBvhNodes(nd, n_nodes, UINT32_MAX, nullptr);      // (no primitive count here: leaf ranges are not checked)
    if (*bad) return SetError(HPRT_E_INVALID, std::string("hprt_debug_wide_build: ") + bad);
    std::vector<int32_t> leafRef(n_nodes, WIDE_NONE);
    for (uint32_t i = 0; i < n_nodes; ++i)
        if ((nd[i].countAxis & 3u) == 3u) leafRef[i] = (int32_t)(~(uint32_t)nd[i].offset & ~WIDE_LEAF_BOXED);
    std::vector<DevWide> wide;
    if (!BuildWide(nd, n_nodes, leafRef.data(), &wide, stack_need)) return SetError(HPRT_E_UNSUPPORTED, "the tree does not fit the four-wide grid");
    *n_out = wide.size();
    if (out64 && cap >= wide.size()) memcpy(out64, wide.data(), wide.size() * sizeof(DevWide));
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }

// Diagnostics hook (not part of include/hprt.h; tests/test_shape_inline_host.py): BuildSceneLayout on a description, no device.  Per
// ordered primitive the tag word of its record and the word beside it (the shape of a triangle or sphere), per shape the flags and the
// material index of its DevShape.  A null or short array is not written; the counts always are.
__attribute__((visibility("default"))) int hprt_debug_shape_inline(const HprtSceneDesc *d, uint32_t *tags, uint32_t *prim_shape, size_t prim_cap, size_t *n_prims,
                                                                    uint32_t *shape_flags, int32_t *shape_material, size_t shape_cap, size_t *n_shapes) try {
    if (!d || !n_prims || !n_shapes) return SetError(HPRT_E_INVALID, "hprt_debug_shape_inline: null argument");
    std::vector<uint32_t> t, ps, sf;
    std::vector<int32_t> smat;
    if (int rc = LayoutTagsForDebug(*d, &t, &ps, &sf, &smat)) return rc;
    *n_prims = t.size(); *n_shapes = sf.size();
    if (tags && prim_shape && prim_cap >= t.size()) { memcpy(tags, t.data(), 4 * t.size()); memcpy(prim_shape, ps.data(), 4 * ps.size()); }
    if (shape_flags && shape_material && shape_cap >= sf.size()) { memcpy(shape_flags, sf.data(), 4 * sf.size()); memcpy(shape_material, smat.data(), 4 * smat.size()); }
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }

// The triangles of the grid hooks below: n triangles given as [n][9] floats, as 12 floats per triangle, each a leaf of its own, and
// their bound.  The point grid's hooks take the min / max of all coordinates as they compare (finiteOnly = false, no bound6); the
// distant grid's skip the coordinates that are not finite, and take bound6 = {min, max} instead if it is given.
struct GridHookTriangles {
    std::vector<float> tris;
    std::vector<uint8_t> single;
    float lo[3] = {HPRT_INF, HPRT_INF, HPRT_INF}, hi[3] = {-HPRT_INF, -HPRT_INF, -HPRT_INF};
    GridHookTriangles(size_t n, const float *p9, bool finiteOnly, const float *bound6) : tris(12 * n, 0.f), single(n, 1) {
        for (size_t i = 0; i < n; ++i)
            for (int v = 0; v < 3; ++v)
                for (int a = 0; a < 3; ++a) {
                    const float x = p9[9 * i + 3 * v + a];
                    tris[12 * i + 4 * v + a] = x;
                    if (finiteOnly && !std::isfinite(x)) continue;
                    if (x < lo[a]) lo[a] = x;
                    if (x > hi[a]) hi[a] = x;
                }
        if (bound6) for (int a = 0; a < 3; ++a) { lo[a] = bound6[a]; hi[a] = bound6[3 + a]; }
    }
};
// info[0 .. 6) = {R, entries, near-list length, eps, longest list, build seconds}; cell_start and entries ({primitive word, key bits}
// pairs) are written when they fit their capacities (counted in words and pairs)
static void GridHookLists(const ShadowGrid &g, double *info, uint32_t *cell_start, size_t cell_cap, uint32_t *entries, size_t entry_cap) {
    info[0] = g.R; info[1] = (double)g.entries.size(); info[2] = g.nNear; info[3] = g.eps; info[4] = g.longest; info[5] = g.buildSeconds;
    if (cell_start && cell_cap >= g.cellStart.size()) memcpy(cell_start, g.cellStart.data(), 4 * g.cellStart.size());
    if (entries && entry_cap >= g.entries.size()) memcpy(entries, g.entries.data(), 8 * g.entries.size());
}
// The device image (shadow_grid.h, ShadowGridImage) of g: words3 = {block words, record words with the padding, what
// ShadowGridImageBytes says of the grid}; each array is written when it fits its capacity in words.
static void GridHookImage(const ShadowGrid &g, const float *tris, size_t words3[3], uint32_t *blocks, size_t block_cap, uint32_t *records, size_t record_cap) {
    ShadowGridImage im;
    PackShadowGrid(g, tris, &im);
    words3[0] = im.blocks.size(); words3[1] = im.records.size(); words3[2] = ShadowGridImageBytes(g) / sizeof(uint32_t);
    if (blocks && block_cap >= im.blocks.size()) memcpy(blocks, im.blocks.data(), 4 * im.blocks.size());
    if (records && record_cap >= im.records.size()) memcpy(records, im.records.data(), 4 * im.records.size());
}

// Diagnostics hook (not part of include/hprt.h; tests/test_shadow_grid_host.py): BuildShadowGrid, no device, on n triangles around
// `light`, over the bound of the triangles.  info6 and the arrays (cell_start: 6 R^2 + 1 words): GridHookLists.
__attribute__((visibility("default"))) int hprt_debug_shadow_grid_build(size_t n, const float *p9, const float light[3], uint32_t R, double info6[6],
                                                                         uint32_t *cell_start, size_t cell_cap, uint32_t *entries, size_t entry_cap) try {
    if (!n || !p9 || !light || !info6 || R == 0 || n >= (1u << 28)) return SetError(HPRT_E_INVALID, "hprt_debug_shadow_grid_build: bad argument");
    const GridHookTriangles t(n, p9, false, nullptr);
    ShadowGrid g;
    BuildShadowGrid(t.tris.data(), t.single.data(), (uint32_t)n, light, t.lo, t.hi, R, (size_t)1 << 27, 0.0, &g);
    if (!g.eligible) return SetError(HPRT_E_UNSUPPORTED, "hprt_debug_shadow_grid_build: the lists do not fit");
    GridHookLists(g, info6, cell_start, cell_cap, entries, entry_cap);
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }

// Diagnostics hook (not part of include/hprt.h; tests/test_shadow_grid_blocks_host.py): the device image of the grid that
// hprt_debug_shadow_grid_build builds of the same arguments, no device.  words3 and the arrays: GridHookImage.
__attribute__((visibility("default"))) int hprt_debug_shadow_grid_image(size_t n, const float *p9, const float light[3], uint32_t R, size_t words3[3],
                                                                         uint32_t *blocks, size_t block_cap, uint32_t *records, size_t record_cap) try {
    if (!n || !p9 || !light || !words3 || R == 0 || n >= (1u << 28)) return SetError(HPRT_E_INVALID, "hprt_debug_shadow_grid_image: bad argument");
    const GridHookTriangles t(n, p9, false, nullptr);
    ShadowGrid g;
    BuildShadowGrid(t.tris.data(), t.single.data(), (uint32_t)n, light, t.lo, t.hi, R, (size_t)1 << 27, 0.0, &g);
    if (!g.eligible || g.R != R) return SetError(HPRT_E_UNSUPPORTED, "hprt_debug_shadow_grid_image: the lists do not fit");
    GridHookImage(g, t.tris.data(), words3, blocks, block_cap, records, record_cap);
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }

// Diagnostics hook (not part of include/hprt.h; tests/test_distant_grid_host.py): BuildDistantGrid, no device, on n triangles under
// the light direction w, over bound6 (null: the bound of the triangles).  info22 = {GridHookLists' six, footprint margin, height
// margin, U[3], V[3], W[3], u0, v0, scaleU, scaleV, hTop}; the arrays (cell_start: R^2 + 1 words): GridHookLists.
__attribute__((visibility("default"))) int hprt_debug_distant_grid_build(size_t n, const float *p9, const float w[3], const float *bound6, uint32_t R, double info22[22],
                                                                          uint32_t *cell_start, size_t cell_cap, uint32_t *entries, size_t entry_cap) try {
    if (!n || !p9 || !w || !info22 || R == 0 || n >= (1u << 28)) return SetError(HPRT_E_INVALID, "hprt_debug_distant_grid_build: bad argument");
    const GridHookTriangles t(n, p9, true, bound6);
    DistantGrid dg;
    BuildDistantGrid(t.tris.data(), t.single.data(), (uint32_t)n, w, t.lo, t.hi, R, (size_t)1 << 27, 0.0, &dg);
    if (!dg.lists.eligible) return SetError(HPRT_E_UNSUPPORTED, "hprt_debug_distant_grid_build: the lists do not fit, or the direction or the bound is not usable");
    GridHookLists(dg.lists, info22, cell_start, cell_cap, entries, entry_cap);
    info22[6] = dg.margin; info22[7] = dg.heightMargin;
    const DgFrame &f = dg.frame;
    for (int a = 0; a < 3; ++a) { info22[8 + a] = f.U[a]; info22[11 + a] = f.V[a]; info22[14 + a] = f.W[a]; }
    info22[17] = f.u0; info22[18] = f.v0; info22[19] = f.scaleU; info22[20] = f.scaleV; info22[21] = f.hTop;
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }

// Diagnostics hook (not part of include/hprt.h; tests/test_distant_grid_host.py): the device image of the grid that
// hprt_debug_distant_grid_build builds of the same arguments, no device.  words3 and the arrays: GridHookImage.
__attribute__((visibility("default"))) int hprt_debug_distant_grid_image(size_t n, const float *p9, const float w[3], const float *bound6, uint32_t R, size_t words3[3],
                                                                          uint32_t *blocks, size_t block_cap, uint32_t *records, size_t record_cap) try {
    if (!n || !p9 || !w || !words3 || R == 0 || n >= (1u << 28)) return SetError(HPRT_E_INVALID, "hprt_debug_distant_grid_image: bad argument");
    const GridHookTriangles t(n, p9, true, bound6);
    DistantGrid dg;
    BuildDistantGrid(t.tris.data(), t.single.data(), (uint32_t)n, w, t.lo, t.hi, R, (size_t)1 << 27, 0.0, &dg);
    if (!dg.lists.eligible || dg.lists.R != R) return SetError(HPRT_E_UNSUPPORTED, "hprt_debug_distant_grid_image: the lists do not fit");
    GridHookImage(dg.lists, t.tris.data(), words3, blocks, block_cap, records, record_cap);
    return HPRT_OK;
} catch (...) { return hprt::HandleException(); }

}  // extern "C"
