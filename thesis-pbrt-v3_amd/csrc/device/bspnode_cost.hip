// hprt — k_sweepcost: the candidates of one node-based BSP build node costed on gfx950, one candidate per lane (bspnode_cost.h:
// the cut, the two surface areas over the child's directions and the cost formula of the candidate's direction, the same code the
// host runs).  A translation unit of its own with a pinned CUID (build.py), so that the other code objects stay byte for byte
// what they were.
//
// The shape is k_bspcost's axis kernel.  Workgroups of one wave; the node's mesh, its direction list and the compact direction
// table are staged in LDS once per workgroup and read as broadcasts.  What depends on a sweep direction alone (DirectionId, its
// place in the compact table, whether it enters it, the kind of its formula) is computed once per workgroup by lanes 0..nDirs-1
// into a table in LDS that every candidate reads as a broadcast, so a candidate is one 16-byte load.  A lane's two half-meshes and
// its face vertices live in a workspace in HBM laid out [word][lane], sized by the lanes in flight (grid-stride loop over the
// candidates), allocated at the build's first node and again only when a later node needs more lanes; the edge list of the face
// being chained is per lane in LDS, [entry][lane].  Nothing per lane is a run-time-indexed private array, so the kernels use no
// scratch.  FASTKD selects the kinds 1 and 2 and the store of the fixed costs.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <string>
#include "../../../include/hprt.h"
#include "../bspnode_cost_device.h"
#include "cost_session.h"

namespace hprt {
namespace {

using namespace bspnodecost;
using bspcost::BitsF;

template <bool FASTKD>
__global__ __launch_bounds__(64) void k_sweepcost(Node nd, Scalars sc, const SweepDir *__restrict__ sweep, uint32_t nDirs, const Cand *__restrict__ cands,
                                                  uint32_t n, uint32_t capEdges, uint32_t capFaces, uint32_t capFaceEdges, Q *__restrict__ ws, uint32_t lanes,
                                                  float *__restrict__ costs, float *__restrict__ costsFixed, uint8_t *__restrict__ overflow) {
    __shared__ Edge sMesh[BSP_MAX_EDGES];
    __shared__ float sDirs[3 * BSP_MAX_DIRS];
    __shared__ uint32_t sCdir[BSP_MAX_FACES / 2];
    __shared__ uint8_t sList[BSP_MAX_FACE_EDGES * kWave];
    __shared__ Dir sTable[BSPNODE_MAX_SWEEP_DIRS];
    // (the launcher has checked; never index past LDS or the workspace)
    if (nd.nE > BSP_MAX_EDGES || nd.M > BSP_MAX_DIRS || nd.nD > BSP_MAX_FACES / 2 || nDirs > BSPNODE_MAX_SWEEP_DIRS || capEdges > BSP_MAX_EDGES ||
        capFaces > BSP_MAX_FACES || capFaceEdges > BSP_MAX_FACE_EDGES)
        return;
    for (uint32_t k = threadIdx.x; k < nd.nE; k += kWave) sMesh[k] = nd.mesh[k];
    for (uint32_t k = threadIdx.x; k < 3 * nd.M; k += kWave) sDirs[k] = nd.dirs[k];
    for (uint32_t k = threadIdx.x; k < nd.nD; k += kWave) sCdir[k] = nd.cdir[k];
    __syncthreads();
    nd.mesh = sMesh; nd.dirs = sDirs; nd.cdir = sCdir;
    if (threadIdx.x < nDirs) {
        const Q s = reinterpret_cast<const Q *>(sweep)[threadIdx.x];
        SweepDir sd;
        sd.axis[0] = BitsF(s.x); sd.axis[1] = BitsF(s.y); sd.axis[2] = BitsF(s.z); sd.kind = s.w;
        sTable[threadIdx.x] = PrepareDir(nd, sd);
    }
    __syncthreads();
    const uint32_t g = blockIdx.x * kWave + threadIdx.x;
    if (g >= lanes) return;
    Store st;
    st.left = ws + g;
    st.right = ws + (size_t)(2 * BSP_MAX_EDGES) * lanes + g;
    st.fv = ws + (size_t)(4 * BSP_MAX_EDGES) * lanes + g;
    st.stride = lanes;
    st.flist = sList + threadIdx.x;
    st.fstride = kWave;
    st.stack = nullptr;
    st.sstride = 0;
    st.capEdges = capEdges; st.capFaces = capFaces; st.capFaceEdges = capFaceEdges; st.capStack = 0u;
    for (uint32_t j = g; j < n; j += gridDim.x * kWave) {
        const Q cq = reinterpret_cast<const Q *>(cands)[j];
        Cand c;
        c.k = cq.x; c.nBelow = cq.y; c.nAbove = cq.z; c.t = BitsF(cq.w);
        float cost = 0, costFixed = bspcost::Inf();
        uint8_t ovf = 1;
        if (c.k < nDirs) {
            // (field by field: the table's entry stays in registers)
            const Dir &e = sTable[c.k];
            Dir d;
            d.axis[0] = e.axis[0]; d.axis[1] = e.axis[1]; d.axis[2] = e.axis[2]; d.kind = e.kind; d.id = e.id; d.p = e.p; d.entered = e.entered; d.pad = 0;
            CostCandidate<FASTKD>(nd, sc, d, c, st, &cost, &costFixed, &ovf);
        }
        costs[j] = cost;
        if (FASTKD) costsFixed[j] = costFixed;
        overflow[j] = ovf;
    }
}

}  // namespace

// hIn: mesh, directions, compact table, sweep directions, candidates; hOut: costs, costsFixed, overflow
struct BspNodeCostDevice : CostSession {
    uint32_t cap[3] = {BSP_MAX_EDGES, BSP_MAX_FACES, BSP_MAX_FACE_EDGES};
};

int BspNodeCostDeviceCreate(int device, const uint32_t caps[3], BspNodeCostDevice **out, std::string *err) {
    *out = nullptr;
    int n = 0;
    if (const int rc = CostDeviceCount(&n, err)) return rc;
    Scalars sc{};
    sc.maxEdges = caps[0]; sc.maxFaces = caps[1]; sc.maxFaceEdges = caps[2];
    uint32_t cap[4];
    if (!bspcost::Capacities(sc, cap)) {
        *err = "max_edges / max_faces / max_face_edges may only lower the compiled capacities (" + std::to_string(BSP_MAX_EDGES) + ", " +
               std::to_string(BSP_MAX_FACES) + ", " + std::to_string(BSP_MAX_FACE_EDGES) + ")";
        return HPRT_E_INVALID;
    }
    BspNodeCostDevice *d = new BspNodeCostDevice();
    for (int k = 0; k < 3; ++k) d->cap[k] = cap[k];
    if (const int rc = d->Open(device, n, err)) { delete d; return rc; }
    *out = d;
    return HPRT_OK;
}

void BspNodeCostDeviceDestroy(BspNodeCostDevice *d) { CostSessionDestroy(d); }

int BspNodeCostDeviceRun(BspNodeCostDevice *d, const Edge *mesh, uint32_t nE, const float *dirs, uint32_t M, const uint32_t *cdir, uint32_t nD, bool fastKd,
                         const Scalars &sc, const SweepDir *sweep, uint32_t nDirs, const Cand *cands, size_t n, float *costs, float *costsFixed,
                         uint8_t *overflow, std::string *err) {
    if (n == 0) return HPRT_OK;
    if (nE > d->cap[0] || M > BSP_MAX_DIRS || M == 0 || 2 * nD > d->cap[1] || nD > M || n > 0x7fffffffull || nDirs == 0 || nDirs > BSPNODE_MAX_SWEEP_DIRS ||
        (fastKd && !costsFixed)) {
        *err = "k_sweepcost: a mesh, a direction list, a sweep or a candidate list beyond the kernel's bounds"; return HPRT_E_INVALID;
    }
#define BSPNODE_TRY(x) COST_TRY("k_sweepcost", x)
    BSPNODE_TRY(hipSetDevice(d->device));
    // staging layout (16-byte aligned parts): in = mesh | directions | compact table | sweep directions | candidates;
    // out = costs | costsFixed (fastKd) | overflow
    const size_t meshBytes = (size_t)BSP_MAX_EDGES * sizeof(Edge), dirBytes = Pad16((size_t)BSP_MAX_DIRS * 12), cdirBytes = Pad16((size_t)BSP_MAX_FACES * 2);
    const size_t sweepBytes = (size_t)BSPNODE_MAX_SWEEP_DIRS * sizeof(SweepDir), candBytes = n * sizeof(Cand);
    const size_t offDirs = meshBytes, offCdir = offDirs + dirBytes, offSweep = offCdir + cdirBytes, offCands = offSweep + sweepBytes, inBytes = offCands + candBytes;
    const size_t costBytes = Pad16(n * 4), offOvf = (fastKd ? 2 : 1) * costBytes, outBytes = offOvf + n;
    const uint32_t lanes = d->Lanes(n);
    // the first node that fills the device sizes the workspace for the build: (4 BSP_MAX_EDGES + 2 BSP_MAX_FACES) words a lane
    BSPNODE_TRY(d->Reserve(inBytes, outBytes, lanes, bspcost::kStoreWords * sizeof(Q), false));
    char *h = (char *)d->hIn.p;
    if (nE) std::memcpy(h, mesh, (size_t)nE * sizeof(Edge));
    std::memcpy(h + offDirs, dirs, (size_t)3 * M * 4);
    if (nD) std::memcpy(h + offCdir, cdir, (size_t)nD * 4);
    std::memcpy(h + offSweep, sweep, (size_t)nDirs * sizeof(SweepDir));
    std::memcpy(h + offCands, cands, candBytes);
    BSPNODE_TRY(d->Upload(inBytes));
    char *di = (char *)d->dIn.p, *dO = (char *)d->dOut.p;
    Node nd{};
    nd.mesh = (const Edge *)di; nd.nE = nE; nd.dirs = (const float *)(di + offDirs); nd.M = M; nd.cdir = (const uint32_t *)(di + offCdir); nd.nD = nD;
    float *dCosts = (float *)dO, *dFixed = fastKd ? (float *)(dO + costBytes) : nullptr;
    uint8_t *dOvf = (uint8_t *)(dO + offOvf);
    // the layout of the workspace uses the lanes of the launch as its stride: every launch owns the whole workspace
    if (fastKd)
        hipLaunchKernelGGL(k_sweepcost<true>, dim3(lanes / kWave), dim3(kWave), 0, d->stream, nd, sc, (const SweepDir *)(di + offSweep), nDirs,
                           (const Cand *)(di + offCands), (uint32_t)n, d->cap[0], d->cap[1], d->cap[2], (Q *)d->ws.p, lanes, dCosts, dFixed, dOvf);
    else
        hipLaunchKernelGGL(k_sweepcost<false>, dim3(lanes / kWave), dim3(kWave), 0, d->stream, nd, sc, (const SweepDir *)(di + offSweep), nDirs,
                           (const Cand *)(di + offCands), (uint32_t)n, d->cap[0], d->cap[1], d->cap[2], (Q *)d->ws.p, lanes, dCosts, dFixed, dOvf);
    BSPNODE_TRY(hipGetLastError());
    BSPNODE_TRY(d->Download(outBytes));
#undef BSPNODE_TRY
    const char *o = (const char *)d->hOut.p;
    std::memcpy(costs, o, n * 4);
    if (fastKd) std::memcpy(costsFixed, o + costBytes, n * 4);
    std::memcpy(overflow, o + offOvf, n);
    return HPRT_OK;
}

}  // namespace hprt
