// hprt — host interface of the device build of the HLBVH form of Accelerator "bvhold" (device/hlbvh_build.hip): centroid
// bounds, Morton codes, radix sort, treelet intervals and emitLBVH as gfx950 kernels behind a launcher that owns the device
// buffers, the pinned staging and the stream of one build; the upper SAH and the final array are bvhold_builder.cpp's.
// capi_host.cpp drives it (hprt_bvhold_build_device).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include "../../include/hprt.h"
#include "bvhold_builder.h"

namespace hprt {

struct HlbvhDevice;      // one per build call, reused across a model's trees

constexpr uint32_t kHlbvhSerialTreeletDefault = 4096;     // the largest treelet one lane emits, by default
constexpr uint32_t kHlbvhSerialTreeletCap = 65536;        // and at most: a leaf may not reach kBvhOldMaxLeaf
// The most primitives of one tree: what k_radix_scan, ONE workgroup over the [256][n / 2048] table, still walks in 4,096 steps of
// 2,048 entries a pass (and 4 GB of treelet nodes); a larger tree is refused, its build is hprt_bvhold_build's
constexpr size_t kHlbvhMaxPrims = (size_t)1 << 26;

// How many HIP devices there are: HPRT_OK, or HPRT_E_NO_DEVICE with the message in *err
int HlbvhDeviceCount(int *n, std::string *err);
// HPRT_OK, or HPRT_E_NO_DEVICE / HPRT_E_INVALID / HPRT_E_DEVICE with the message in *err, in this order: no device, the
// capacity (serialTreeletMax may only lower kHlbvhSerialTreeletCap; 0 = the default), the ordinal.  device < 0: the current device.
int HlbvhDeviceCreate(int device, uint32_t serialTreeletMax, HlbvhDevice **out, std::string *err);
void HlbvhDeviceDestroy(HlbvhDevice *d);
// The HLBVH tree of n primitives (n <= kHlbvhMaxPrims: the caller has checked), byte for byte BuildBvhOld's with BVHOLD_HLBVH.
// HPRT_OK, HPRT_E_UNSUPPORTED (BuildBvhOld's refusals) or HPRT_E_DEVICE; stats (may be null) are added to.
int HlbvhDeviceBuild(HlbvhDevice *d, size_t n, const float *bmin, const float *bmax, int maxNodePrims, BvhTree *out, HprtBvhOldDeviceStats *stats,
                     std::string *err);

}  // namespace hprt
