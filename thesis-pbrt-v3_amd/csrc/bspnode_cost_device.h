// hprt — host interface of the device-side costing of node-based BSP split candidates (device/bspnode_cost.hip): k_sweepcost
// behind a launcher that owns the per-lane workspace, the pinned staging buffers and the stream.  capi_host.cpp drives it from the
// node-based builder's costing hook.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include "bspnode_cost.h"

namespace hprt {

struct BspNodeCostDevice;       // one per build, reused across its nodes

// HPRT_OK, or HPRT_E_NO_DEVICE / HPRT_E_INVALID / HPRT_E_DEVICE with the message in *err.  device < 0: the current device.
// caps: maxEdges, maxFaces, maxFaceEdges; 0 = the compiled capacity, else it lowers it.
int BspNodeCostDeviceCreate(int device, const uint32_t caps[3], BspNodeCostDevice **out, std::string *err);
void BspNodeCostDeviceDestroy(BspNodeCostDevice *d);
// One node.  mesh: nE edges with compact face ids, cdir: the nD directions that own a face (bspcost::CompactNode); sweep: the
// nDirs <= BSPNODE_MAX_SWEEP_DIRS directions of the sweep; cands: n candidates, each k below nDirs.  The caller has checked nE, nD,
// M and nDirs against the capacities and every index of the mesh and the candidates.  Writes costs, costsFixed (fastKd only; may
// be NULL otherwise) and overflow for every candidate.  HPRT_OK, HPRT_E_INVALID or HPRT_E_DEVICE.
int BspNodeCostDeviceRun(BspNodeCostDevice *d, const bspcost::Edge *mesh, uint32_t nE, const float *dirs, uint32_t M, const uint32_t *cdir, uint32_t nD,
                         bool fastKd, const bspcost::Scalars &sc, const bspnodecost::SweepDir *sweep, uint32_t nDirs, const bspnodecost::Cand *cands,
                         size_t n, float *costs, float *costsFixed, uint8_t *overflow, std::string *err);

}  // namespace hprt
