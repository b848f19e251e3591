// hprt — host interface of the device-side costing of general BSP split candidates (device/bsp_cost.hip): k_bspcost behind a
// launcher that owns the build's primitive arrays on the device, the per-lane workspace, the pinned staging buffers and the
// stream.  capi_host.cpp drives it from the bsppaper builder's costing hook.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include "bsp_cost.h"

namespace hprt {

struct BspCostDevice;       // one per build, reused across its nodes

// HPRT_OK, or HPRT_E_NO_DEVICE / HPRT_E_INVALID / HPRT_E_DEVICE with the message in *err.  device < 0: the current device.
// caps: maxEdges, maxFaces, maxFaceEdges, maxStack; 0 = the compiled capacity, else it lowers it.  The primitives' bmin / bmax /
// tri9 / isTri (nTotal of them) are uploaded here, once.
int BspCostDeviceCreate(int device, const uint32_t caps[4], size_t nTotal, const float *bmin, const float *bmax, const float *tri9,
                        const uint8_t *isTri, BspCostDevice **out, std::string *err);
void BspCostDeviceDestroy(BspCostDevice *d);
// One node.  mesh: nE edges with compact face ids, cdir: the nD directions that own a face (bspcost::CompactNode); cands: n
// candidates, the first nAxis of them axis candidates and the rest plane candidates; bvh / primOrder / primNums: the node's BVH
// (nBvh records, nPrims primitives; unused when n == nAxis).  The caller has checked nE, nD and M against the capacities and
// every index of the mesh.  Writes costs, costsFixed (+inf unless a kd-aware plane inside the extent), counts (2 per candidate:
// nBelow, nAbove) and overflow for every candidate.  HPRT_OK, HPRT_E_INVALID or HPRT_E_DEVICE.
int BspCostDeviceRun(BspCostDevice *d, const bspcost::Edge *mesh, uint32_t nE, const float *dirs, uint32_t M, const uint32_t *cdir, uint32_t nD,
                     bool kdAware, const bspcost::Scalars &sc, const bspcost::Cand *cands, size_t n, size_t nAxis, const bspcost::BvhRec *bvh,
                     uint32_t nBvh, const uint32_t *primOrder, const uint32_t *primNums, uint32_t nPrims, float *costs, float *costsFixed,
                     uint32_t *counts, uint8_t *overflow, std::string *err);

}  // namespace hprt
