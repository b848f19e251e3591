// hprt — host interface of the device-side candidate costing (device/kdop_cost.hip): k_kdopcost behind a launcher that owns the
// per-build device workspace and the pinned staging buffers.  capi_host.cpp drives it from the RBSP builder's costing hook.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include "kdop_cost.h"

namespace hprt {

struct KdopCostDevice;      // device buffers, pinned staging, stream: one per build, reused across its nodes

// HPRT_OK, or HPRT_E_NO_DEVICE / HPRT_E_INVALID / HPRT_E_DEVICE with the message in *err.  device < 0: the current device.
// maxEdges: 0 = KDOP_MAX_EDGES, else it lowers the capacity of a half-mesh (and of a node's mesh).
int KdopCostDeviceCreate(int device, uint32_t maxEdges, KdopCostDevice **out, std::string *err);
void KdopCostDeviceDestroy(KdopCostDevice *d);
uint32_t KdopCostDeviceCapacity(const KdopCostDevice *d);
// Costs n candidates of one mesh (nE <= the capacity, M in {3, 7, 9, 13}, every face id < 2 M, every candidate's d < M: the
// caller has checked).  costsFixed is written only when kdAware.  HPRT_OK or HPRT_E_DEVICE.
int KdopCostDeviceRun(KdopCostDevice *d, const kdopcost::Edge *mesh, uint32_t nE, const float *dirs, uint32_t M, bool kdAware,
                      const kdopcost::Scalars &sc, const kdopcost::Cand *cands, size_t n, float *costs, float *costsFixed, uint8_t *overflow,
                      std::string *err);

}  // namespace hprt
