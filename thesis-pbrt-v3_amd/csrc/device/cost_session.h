// hprt — what the launchers of the three costing kernels share (kdop_cost.hip, bsp_cost.hip, bspnode_cost.hip): the device, the
// stream, the pinned staging buffers, the device buffers and the per-lane workspace of one build.  Host code only; each unit keeps
// its own capacities, staging layout and launches.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include "../../../include/hprt.h"

namespace hprt {

constexpr uint32_t kWave = 64;
constexpr uint32_t kWavesPerCU = 8;      // lanes in flight = CUs * kWavesPerCU * 64 at most

struct Pinned {
    void *p = nullptr; size_t bytes = 0;
    hipError_t reserve(size_t b) {
        if (b <= bytes) return hipSuccess;
        if (p) (void)hipHostFree(p);
        p = nullptr; bytes = 0;
        b = std::max<size_t>(b + b / 2, 4096);
        hipError_t e = hipHostMalloc(&p, b, hipHostMallocDefault);
        if (e == hipSuccess) bytes = b; else p = nullptr;
        return e;
    }
    ~Pinned() { if (p) (void)hipHostFree(p); }
};
struct Dev {
    void *p = nullptr; size_t bytes = 0;
    hipError_t reserve(size_t b, bool grow = true) {      // grow: half as much again, for buffers that follow the nodes' sizes
        if (b <= bytes) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr; bytes = 0;
        b = std::max<size_t>(grow ? b + b / 2 : b, 4096);
        hipError_t e = hipMalloc(&p, b);
        if (e == hipSuccess) bytes = b; else p = nullptr;
        return e;
    }
    ~Dev() { if (p) (void)hipFree(p); }
};
constexpr size_t Pad16(size_t b) { return (b + 15) & ~(size_t)15; }

// `return HPRT_E_DEVICE` with "<kernel> launcher: <HIP's message>" in *err when x fails
#define COST_TRY(kernel, x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { *err = std::string(kernel " launcher: ") + hipGetErrorString(e_); return HPRT_E_DEVICE; } } while (0)

// A Create refuses in this order: no device (CostDeviceCount), the unit's capacities, then the ordinal and the rest (Open)
inline int CostDeviceCount(int *n, std::string *err) {
    *n = 0;
    if (hipGetDeviceCount(n) != hipSuccess || *n <= 0) { *err = "no HIP device available (the device-assisted build has no CPU fallback)"; return HPRT_E_NO_DEVICE; }
    return HPRT_OK;
}

// One per build, reused across its nodes
struct CostSession {
    int device = 0;
    uint32_t maxLanes = 0, wsLanes = 0;
    hipStream_t stream = nullptr;
    Pinned hIn, hOut;           // a node's inputs and results, each unit's own layout
    Dev dIn, dOut, ws;
    ~CostSession() { if (stream) (void)hipStreamDestroy(stream); }

    // dev < 0: the current device; nDevices: what CostDeviceCount gave
    int Open(int dev, int nDevices, std::string *err) {
        if (dev < 0) { if (hipGetDevice(&dev) != hipSuccess) dev = 0; }
        if (dev >= nDevices) { *err = "device ordinal out of range"; return HPRT_E_INVALID; }
        if (hipSetDevice(dev) != hipSuccess) { *err = "hipSetDevice failed"; return HPRT_E_DEVICE; }
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) != hipSuccess) { *err = "hipGetDeviceProperties failed"; return HPRT_E_DEVICE; }
        device = dev;
        maxLanes = (uint32_t)std::max(1, prop.multiProcessorCount) * kWavesPerCU * kWave;
        if (hipStreamCreate(&stream) != hipSuccess) { stream = nullptr; *err = "hipStreamCreate failed"; return HPRT_E_DEVICE; }
        return HPRT_OK;
    }
    // The lanes of a launch over n candidates: whole waves, at most what fills the device
    uint32_t Lanes(size_t n) const { return (uint32_t)std::min<size_t>(maxLanes, (n + kWave - 1) / kWave * kWave); }
    // The staging buffers of a node, and a workspace of laneBytes a lane: the first node that needs more lanes sizes it again
    hipError_t Reserve(size_t inBytes, size_t outBytes, uint32_t lanes, size_t laneBytes, bool growWorkspace) {
        hipError_t e = hIn.reserve(inBytes);
        if (e == hipSuccess) e = hOut.reserve(outBytes);
        if (e == hipSuccess) e = dIn.reserve(inBytes);
        if (e == hipSuccess) e = dOut.reserve(outBytes);
        if (e == hipSuccess && lanes > wsLanes) {
            e = ws.reserve((size_t)lanes * laneBytes, growWorkspace);
            if (e == hipSuccess) wsLanes = lanes;
        }
        return e;
    }
    hipError_t Upload(size_t inBytes) { return hipMemcpyAsync(dIn.p, hIn.p, inBytes, hipMemcpyHostToDevice, stream); }
    // The results back and the stream drained
    hipError_t Download(size_t outBytes) {
        hipError_t e = hipMemcpyAsync(hOut.p, dOut.p, outBytes, hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        return e;
    }
};

// D: a CostSession with a unit's own fields
template <class D>
void CostSessionDestroy(D *d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    delete d;
}

}  // namespace hprt
