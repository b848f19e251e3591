// hprt — k_bspcost: the candidates of one general BSP build node costed on gfx950, one candidate per lane (bsp_cost.h: the extent
// test, DirectionId, the cut and the two surface areas over the child's directions, NodeBvh::count and the cost formulas of
// BuildBspPaperTree's costRange, the same code the host runs).  A translation unit of its own with a pinned CUID (build.py), so
// that the other code objects stay byte for byte what they were.
//
// The shape is k_kdopcost's.  Workgroups of one wave; the node's mesh, its direction list and the compact direction table are
// staged in LDS once per workgroup and read as broadcasts.  A lane's two half-meshes and its face vertices live in a workspace
// in HBM laid out [word][lane], sized by the lanes in flight (grid-stride loop over the candidates) and allocated once per build.
// The edge list of the face being chained and the BVH stack are per lane in LDS, [entry][lane].  Nothing per lane is a
// run-time-indexed private array, so the kernels use no scratch.  PLANES tells the two contiguous candidate ranges apart (axis
// candidates first, then plane candidates), one launch each: no wave mixes them, so no axis lane idles behind a BVH walk, and
// the axis kernel carries no stack.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <string>
#include "../../../include/hprt.h"
#include "../bsp_cost_device.h"
#include "cost_session.h"

namespace hprt {
namespace {

using namespace bspcost;

template <bool KD_AWARE, bool PLANES>
__global__ __launch_bounds__(64) void k_bspcost(Node nd, Scalars sc, const Cand *__restrict__ cands, uint32_t first, uint32_t n, uint32_t capEdges,
                                                uint32_t capFaces, uint32_t capFaceEdges, uint32_t capStack, Q *__restrict__ ws, uint32_t lanes,
                                                float *__restrict__ costs, float *__restrict__ costsFixed, uint32_t *__restrict__ counts,
                                                uint8_t *__restrict__ overflow) {
    __shared__ Edge sMesh[BSP_MAX_EDGES];
    __shared__ float sDirs[3 * BSP_MAX_DIRS];
    __shared__ uint32_t sCdir[BSP_MAX_FACES / 2];
    __shared__ uint8_t sList[BSP_MAX_FACE_EDGES * kWave];
    __shared__ uint32_t sStack[(PLANES ? BSP_MAX_STACK : 1) * kWave];
    // (the launcher has checked; never index past LDS or the workspace)
    if (nd.nE > BSP_MAX_EDGES || nd.M > BSP_MAX_DIRS || nd.nD > BSP_MAX_FACES / 2 || capEdges > BSP_MAX_EDGES || capFaces > BSP_MAX_FACES ||
        capFaceEdges > BSP_MAX_FACE_EDGES || capStack > BSP_MAX_STACK)
        return;
    for (uint32_t k = threadIdx.x; k < nd.nE; k += kWave) sMesh[k] = nd.mesh[k];
    for (uint32_t k = threadIdx.x; k < 3 * nd.M; k += kWave) sDirs[k] = nd.dirs[k];
    for (uint32_t k = threadIdx.x; k < nd.nD; k += kWave) sCdir[k] = nd.cdir[k];
    __syncthreads();
    const uint32_t g = blockIdx.x * kWave + threadIdx.x;
    if (g >= lanes) return;
    nd.mesh = sMesh; nd.dirs = sDirs; nd.cdir = sCdir;
    // The pointers that only the BVH walk and the final stores read would sit in SGPRs across every loop of the cut and spill
    // there.  Occupancy is bound by LDS, so VGPRs are spare: an empty asm moves them over (no instruction is emitted).
    if (PLANES) {
        asm volatile("" : "+v"(nd.bvh), "+v"(nd.primOrder), "+v"(nd.primNums));
        asm volatile("" : "+v"(nd.bmin), "+v"(nd.bmax), "+v"(nd.tri9), "+v"(nd.isTri));
        asm volatile("" : "+v"(costs), "+v"(costsFixed), "+v"(counts), "+v"(overflow));
    }
    Store st;
    st.left = ws + g;
    st.right = ws + (size_t)(2 * BSP_MAX_EDGES) * lanes + g;
    st.fv = ws + (size_t)(4 * BSP_MAX_EDGES) * lanes + g;
    st.stride = lanes;
    st.flist = sList + threadIdx.x;
    st.fstride = kWave;
    st.stack = sStack + threadIdx.x;
    st.sstride = kWave;
    st.capEdges = capEdges; st.capFaces = capFaces; st.capFaceEdges = capFaceEdges; st.capStack = PLANES ? capStack : 0u;
    for (uint32_t j = g; j < n; j += gridDim.x * kWave) {
        const uint32_t k = first + j;
        // (two 16-byte loads, field by field: a struct copy would keep the candidate in private memory)
        const Q ca = reinterpret_cast<const Q *>(cands)[2 * (size_t)k], cb = reinterpret_cast<const Q *>(cands)[2 * (size_t)k + 1];
        Cand c;
        c.k = ca.x; c.i = ca.y; c.nBelow = ca.z; c.nAbove = ca.w;
        c.t = BitsF(cb.x); c.axis[0] = BitsF(cb.y); c.axis[1] = BitsF(cb.z); c.axis[2] = BitsF(cb.w);
        float cost = 0, costFixed = Inf();
        uint32_t nBelow = c.nBelow, nAbove = c.nAbove;
        uint8_t ovf = 1;
        if ((c.k == 33u) == PLANES) CostCandidate(nd, KD_AWARE, sc, c, st, &cost, &costFixed, &nBelow, &nAbove, &ovf);
        costs[k] = cost;
        costsFixed[k] = costFixed;
        counts[2 * k] = nBelow; counts[2 * k + 1] = nAbove;
        overflow[k] = ovf;
    }
}

}  // namespace

// hIn: mesh, directions, compact table, candidates, BVH, primOrder, primNums; hOut: costs, costsFixed, counts, overflow
struct BspCostDevice : CostSession {
    uint32_t cap[4] = {BSP_MAX_EDGES, BSP_MAX_FACES, BSP_MAX_FACE_EDGES, BSP_MAX_STACK};
    uint32_t nTotal = 0;
    Dev prims;                  // bmin | bmax | tri9 | isTri of the whole build
    size_t offBmax = 0, offTri9 = 0, offIsTri = 0;
};

int BspCostDeviceCreate(int device, const uint32_t caps[4], size_t nTotal, const float *bmin, const float *bmax, const float *tri9,
                        const uint8_t *isTri, BspCostDevice **out, std::string *err) {
    *out = nullptr;
    int n = 0;
    if (const int rc = CostDeviceCount(&n, err)) return rc;
    Scalars sc{};
    sc.maxEdges = caps[0]; sc.maxFaces = caps[1]; sc.maxFaceEdges = caps[2]; sc.maxStack = caps[3];
    uint32_t cap[4];
    if (!Capacities(sc, cap)) {
        *err = "max_edges / max_faces / max_face_edges / max_stack may only lower the compiled capacities (" + std::to_string(BSP_MAX_EDGES) + ", " +
               std::to_string(BSP_MAX_FACES) + ", " + std::to_string(BSP_MAX_FACE_EDGES) + ", " + std::to_string(BSP_MAX_STACK) + ")";
        return HPRT_E_INVALID;
    }
    if (nTotal > 0x7fffffffull) { *err = "more primitives than the device costing indexes"; return HPRT_E_INVALID; }
    BspCostDevice *d = new BspCostDevice();
    for (int k = 0; k < 4; ++k) d->cap[k] = cap[k];
    d->nTotal = (uint32_t)nTotal;
    if (const int rc = d->Open(device, n, err)) { delete d; return rc; }
    // the primitives, once per build: bmin | bmax | tri9 | isTri
    const size_t b3 = Pad16(nTotal * 12), b9 = Pad16(nTotal * 36);
    d->offBmax = b3; d->offTri9 = 2 * b3; d->offIsTri = 2 * b3 + b9;
    const size_t bytes = d->offIsTri + Pad16(nTotal);
    hipError_t e = d->prims.reserve(bytes, false);
    if (e == hipSuccess) e = d->hIn.reserve(bytes);
    if (e == hipSuccess && nTotal) {
        char *h = (char *)d->hIn.p;
        std::memcpy(h, bmin, nTotal * 12); std::memcpy(h + d->offBmax, bmax, nTotal * 12);
        std::memcpy(h + d->offTri9, tri9, nTotal * 36); std::memcpy(h + d->offIsTri, isTri, nTotal);
        e = hipMemcpyAsync(d->prims.p, h, bytes, hipMemcpyHostToDevice, d->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
    }
    if (e != hipSuccess) { *err = std::string("k_bspcost launcher: ") + hipGetErrorString(e); delete d; return HPRT_E_DEVICE; }
    *out = d;
    return HPRT_OK;
}

void BspCostDeviceDestroy(BspCostDevice *d) { CostSessionDestroy(d); }

int BspCostDeviceRun(BspCostDevice *d, const Edge *mesh, uint32_t nE, const float *dirs, uint32_t M, const uint32_t *cdir, uint32_t nD, bool kdAware,
                     const Scalars &sc, const Cand *cands, size_t n, size_t nAxis, const BvhRec *bvh, uint32_t nBvh, const uint32_t *primOrder,
                     const uint32_t *primNums, uint32_t nPrims, float *costs, float *costsFixed, uint32_t *counts, uint8_t *overflow, std::string *err) {
    if (n == 0) return HPRT_OK;
    const bool planes = nAxis < n;
    if (nE > d->cap[0] || M > BSP_MAX_DIRS || M == 0 || 2 * nD > d->cap[1] || nD > M || n > 0x7fffffffull || nAxis > n || (planes && (nBvh == 0 || nPrims == 0)) ||
        nBvh > 0x7fffffffu) {
        *err = "k_bspcost: a mesh, a direction list, a BVH or a candidate list beyond the kernel's bounds"; return HPRT_E_INVALID;
    }
    if (!planes) { nBvh = 0; nPrims = 0; }
#define BSP_TRY(x) COST_TRY("k_bspcost", x)
    BSP_TRY(hipSetDevice(d->device));
    // staging layout (16-byte aligned parts): in = mesh | directions | compact table | candidates | BVH | primOrder | primNums;
    // out = costs | costsFixed | counts | overflow
    const size_t meshBytes = (size_t)BSP_MAX_EDGES * sizeof(Edge), dirBytes = Pad16((size_t)BSP_MAX_DIRS * 12), cdirBytes = Pad16((size_t)BSP_MAX_FACES * 2);
    const size_t candBytes = n * sizeof(Cand), bvhBytes = (size_t)nBvh * sizeof(BvhRec), idxBytes = Pad16((size_t)nPrims * 4);
    const size_t offDirs = meshBytes, offCdir = offDirs + dirBytes, offCands = offCdir + cdirBytes, offBvh = offCands + candBytes, offOrder = offBvh + bvhBytes,
                 offNums = offOrder + idxBytes, inBytes = offNums + idxBytes;
    const size_t costBytes = Pad16(n * 4), countBytes = Pad16(n * 8);
    const size_t outBytes = 2 * costBytes + countBytes + n;
    const uint32_t lanes = d->Lanes(std::max(nAxis, n - nAxis));      // (the wider of the two launches)
    BSP_TRY(d->Reserve(inBytes, outBytes, lanes, kStoreWords * sizeof(Q), false));
    char *h = (char *)d->hIn.p;
    if (nE) std::memcpy(h, mesh, (size_t)nE * sizeof(Edge));
    std::memcpy(h + offDirs, dirs, (size_t)3 * M * 4);
    if (nD) std::memcpy(h + offCdir, cdir, (size_t)nD * 4);
    std::memcpy(h + offCands, cands, candBytes);
    if (planes) {
        std::memcpy(h + offBvh, bvh, bvhBytes);
        std::memcpy(h + offOrder, primOrder, (size_t)nPrims * 4);
        std::memcpy(h + offNums, primNums, (size_t)nPrims * 4);
    }
    BSP_TRY(d->Upload(inBytes));
    char *di = (char *)d->dIn.p, *dO = (char *)d->dOut.p;
    const char *pr = (const char *)d->prims.p;
    Node nd;
    nd.mesh = (const Edge *)di; nd.nE = nE; nd.dirs = (const float *)(di + offDirs); nd.M = M; nd.cdir = (const uint32_t *)(di + offCdir); nd.nD = nD;
    nd.bvh = (const BvhRec *)(di + offBvh); nd.nBvh = nBvh; nd.primOrder = (const uint32_t *)(di + offOrder); nd.primNums = (const uint32_t *)(di + offNums);
    nd.nPrims = nPrims;
    nd.bmin = (const float *)pr; nd.bmax = (const float *)(pr + d->offBmax); nd.tri9 = (const float *)(pr + d->offTri9);
    nd.isTri = (const uint8_t *)(pr + d->offIsTri); nd.nTotal = d->nTotal;
    float *dCosts = (float *)dO, *dFixed = (float *)(dO + costBytes);
    uint32_t *dCounts = (uint32_t *)(dO + 2 * costBytes);
    uint8_t *dOvf = (uint8_t *)(dO + 2 * costBytes + countBytes);
    // the layout of the workspace uses the lanes of a launch as its stride: every launch owns the whole workspace, and the two
    // launches of a node follow each other on one stream
    auto launch = [&](auto kernel, uint32_t first, uint32_t count) {
        const uint32_t l = d->Lanes(count);      // (at most `lanes`)
        hipLaunchKernelGGL(kernel, dim3(l / kWave), dim3(kWave), 0, d->stream, nd, sc, (const Cand *)(di + offCands), first, count, d->cap[0], d->cap[1],
                           d->cap[2], d->cap[3], (Q *)d->ws.p, l, dCosts, dFixed, dCounts, dOvf);
    };
    if (nAxis) { if (kdAware) launch(k_bspcost<true, false>, 0u, (uint32_t)nAxis); else launch(k_bspcost<false, false>, 0u, (uint32_t)nAxis); }
    BSP_TRY(hipGetLastError());
    if (planes) { if (kdAware) launch(k_bspcost<true, true>, (uint32_t)nAxis, (uint32_t)(n - nAxis)); else launch(k_bspcost<false, true>, (uint32_t)nAxis, (uint32_t)(n - nAxis)); }
    BSP_TRY(hipGetLastError());
    BSP_TRY(d->Download(outBytes));
#undef BSP_TRY
    const char *o = (const char *)d->hOut.p;
    std::memcpy(costs, o, n * 4);
    std::memcpy(costsFixed, o + costBytes, n * 4);
    std::memcpy(counts, o + 2 * costBytes, n * 8);
    std::memcpy(overflow, o + 2 * costBytes + countBytes, n);
    return HPRT_OK;
}

}  // namespace hprt
