// hprt — k_kdopcost: the candidates of one RBSP build node costed on gfx950, one candidate per lane (kdop_cost.h: KDOPCut +
// KDOPSurfaceArea + the cost formulas of BuildRbspTree's costRange, the same code the host runs).  A translation unit of its
// own with a pinned CUID (build.py), so that the other code objects stay byte for byte what they were.
//
// Workgroups of one wave.  The node's mesh (<= KDOP_MAX_EDGES edges of 32 bytes) and the direction table are staged in LDS once
// per workgroup; every lane reads the same edge at the same time (an LDS broadcast).  A lane's two half-meshes and its face
// vertices live in a workspace in HBM, laid out [word][lane] so that a wave's access to one edge is 64 neighbouring 16-byte
// words; the workspace is sized by the lanes in flight (grid-stride loop over the candidates), not by the candidate count.  The
// edge list of the face being chained (KDOP_MAX_FACE_EDGES bytes a lane) is in LDS, [entry][lane].  Nothing per lane is a
// run-time-indexed private array, so the kernels use no scratch.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <string>
#include "../../../include/hprt.h"
#include "../kdop_cost_device.h"
#include "cost_session.h"

namespace hprt {
namespace {

using namespace kdopcost;

template <bool KD_AWARE>
__global__ __launch_bounds__(64) void k_kdopcost(const Edge *__restrict__ mesh, uint32_t nE, const float *__restrict__ dirs, uint32_t M, Scalars sc,
                                                 const Cand *__restrict__ cands, uint32_t n, uint32_t cap, Q *__restrict__ ws, uint32_t lanes,
                                                 float *__restrict__ costs, float *__restrict__ costsFixed, uint8_t *__restrict__ overflow) {
    __shared__ Edge sMesh[KDOP_MAX_EDGES];
    __shared__ float sDirs[3 * 13];
    __shared__ uint8_t sList[KDOP_MAX_FACE_EDGES * kWave];
    if (nE > KDOP_MAX_EDGES || cap > KDOP_MAX_EDGES || nE > cap || M > 13u) return;      // (the launcher has checked; never index past LDS)
    for (uint32_t k = threadIdx.x; k < nE; k += kWave) sMesh[k] = mesh[k];
    for (uint32_t k = threadIdx.x; k < 3 * M; k += kWave) sDirs[k] = dirs[k];
    __syncthreads();
    const uint32_t g = blockIdx.x * kWave + threadIdx.x;
    if (g >= lanes) return;
    Store st;
    st.left = ws + g;
    st.right = ws + (size_t)(2 * KDOP_MAX_EDGES) * lanes + g;
    st.fv = ws + (size_t)(4 * KDOP_MAX_EDGES) * lanes + g;
    st.stride = lanes;
    st.flist = sList + threadIdx.x;
    st.fstride = kWave;
    st.cap = cap;
    for (uint32_t k = g; k < n; k += gridDim.x * kWave) {
        const Cand c = cands[k];
        float cost = 0, costFixed = 0;
        uint8_t ovf = 1;
        if (c.d < M) CostCandidate(sMesh, nE, sDirs, M, KD_AWARE, sc, c, st, &cost, &costFixed, &ovf);
        costs[k] = cost;
        if (KD_AWARE) costsFixed[k] = costFixed;
        overflow[k] = ovf;
    }
}

}  // namespace

struct KdopCostDevice : CostSession {      // hIn: mesh, directions, candidates; hOut: costs, costsFixed, overflow
    uint32_t cap = KDOP_MAX_EDGES;
};

int KdopCostDeviceCreate(int device, uint32_t maxEdges, KdopCostDevice **out, std::string *err) {
    *out = nullptr;
    int n = 0;
    if (const int rc = CostDeviceCount(&n, err)) return rc;
    if (maxEdges > KDOP_MAX_EDGES) { *err = "max_edges may only lower the compiled capacity (" + std::to_string(KDOP_MAX_EDGES) + ")"; return HPRT_E_INVALID; }
    KdopCostDevice *d = new KdopCostDevice();
    d->cap = maxEdges ? maxEdges : KDOP_MAX_EDGES;
    if (const int rc = d->Open(device, n, err)) { delete d; return rc; }
    *out = d;
    return HPRT_OK;
}

void KdopCostDeviceDestroy(KdopCostDevice *d) { CostSessionDestroy(d); }

uint32_t KdopCostDeviceCapacity(const KdopCostDevice *d) { return d->cap; }

int KdopCostDeviceRun(KdopCostDevice *d, const Edge *mesh, uint32_t nE, const float *dirs, uint32_t M, bool kdAware, const Scalars &sc,
                      const Cand *cands, size_t n, float *costs, float *costsFixed, uint8_t *overflow, std::string *err) {
    if (n == 0) return HPRT_OK;
    if (nE > d->cap || M > 13u || n > 0xffffffffull) { *err = "k_kdopcost: a mesh or a candidate list beyond the kernel's bounds"; return HPRT_E_INVALID; }
#define KD_TRY(x) COST_TRY("k_kdopcost", x)
    KD_TRY(hipSetDevice(d->device));
    // staging layout (16-byte aligned parts): in = mesh | directions | candidates; out = costs | costsFixed | overflow
    const size_t meshBytes = (size_t)KDOP_MAX_EDGES * sizeof(Edge), dirBytes = 160, candBytes = n * sizeof(Cand);
    const size_t costBytes = Pad16(n * 4);
    const size_t inBytes = meshBytes + dirBytes + candBytes, outBytes = 2 * costBytes + n;
    const uint32_t lanes = d->Lanes(n);
    KD_TRY(d->Reserve(inBytes, outBytes, lanes, kStoreWords * sizeof(Q), true));
    char *h = (char *)d->hIn.p;
    if (nE) std::memcpy(h, mesh, (size_t)nE * sizeof(Edge));
    std::memcpy(h + meshBytes, dirs, (size_t)3 * M * 4);
    std::memcpy(h + meshBytes + dirBytes, cands, candBytes);
    KD_TRY(d->Upload(inBytes));
    char *di = (char *)d->dIn.p, *dO = (char *)d->dOut.p;
    const dim3 grid(lanes / kWave), block(kWave);
    // the layout of the workspace uses the lanes of THIS launch as its stride: every launch owns the whole workspace
    if (kdAware)
        hipLaunchKernelGGL(k_kdopcost<true>, grid, block, 0, d->stream, (const Edge *)di, nE, (const float *)(di + meshBytes), M, sc,
                           (const Cand *)(di + meshBytes + dirBytes), (uint32_t)n, d->cap, (Q *)d->ws.p, lanes, (float *)dO, (float *)(dO + costBytes),
                           (uint8_t *)(dO + 2 * costBytes));
    else
        hipLaunchKernelGGL(k_kdopcost<false>, grid, block, 0, d->stream, (const Edge *)di, nE, (const float *)(di + meshBytes), M, sc,
                           (const Cand *)(di + meshBytes + dirBytes), (uint32_t)n, d->cap, (Q *)d->ws.p, lanes, (float *)dO, (float *)(dO + costBytes),
                           (uint8_t *)(dO + 2 * costBytes));
    KD_TRY(hipGetLastError());
    KD_TRY(d->Download(outBytes));
#undef KD_TRY
    const char *o = (const char *)d->hOut.p;
    std::memcpy(costs, o, n * 4);
    if (kdAware && costsFixed) std::memcpy(costsFixed, o + costBytes, n * 4);
    std::memcpy(overflow, o + 2 * costBytes, n);
    return HPRT_OK;
}

}  // namespace hprt
