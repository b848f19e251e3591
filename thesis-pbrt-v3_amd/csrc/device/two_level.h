// hprt device side — what the two-level walks share (kdinst_walk.hip; bspinst_walk.h for rbspinst_walk.hip): the per-instance
// entry and the root interval of either level.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels.h"

namespace hprt {

// What a TransformedPrimitive wraps, per instance (32 bytes, two 16-byte reads).  prim < 0: the object's tree — root is its root
// node in the walk's node array (DevKdInst / DevRbspInst::nodes), lo / hi are the accelerator's bounds (KdTreeAccel::bounds,
// GenericBSP::bounds) in object space.  prim >= 0: the object's one primitive, wrapped as it is (core/api.cpp:1798) and tested
// without a bounds test — root is a one-primitive leaf the attach step made for it (its primitive word is prim), which the walk
// enters without counting a node.
struct DevInstEntry { float lo[3]; uint32_t root; float hi[3]; int32_t prim; };
static_assert(sizeof(DevInstEntry) == 32, "DevInstEntry is two 16-byte words");

// Bounds3::IntersectP(const Ray &, Float *hitt0, Float *hitt1) (core/geometry.h:1730-1751): the root interval of either level
// (kd_walk.hip's kd_root_interval and bsp_walk.h's bsp_root_interval over bounds passed by value)
__device__ __forceinline__ bool inst_root_interval(vec3 lo, vec3 hi, vec3 ro, vec3 rd, float rayTMax, float *hitt0, float *hitt1) {
    float t0 = 0, t1 = rayTMax;
    const float robust = 1 + 2 * gamma_n(3);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float invRayDir = 1 / rd.get(i);
        float tNear = (lo.get(i) - ro.get(i)) * invRayDir;
        float tFar = (hi.get(i) - ro.get(i)) * invRayDir;
        if (tNear > tFar) { const float s = tNear; tNear = tFar; tFar = s; }
        tFar *= robust;
        t0 = tNear > t0 ? tNear : t0;
        t1 = tFar < t1 ? tFar : t1;
        if (t0 > t1) return false;
    }
    *hitt0 = t0; *hitt1 = t1;
    return true;
}

}  // namespace hprt
