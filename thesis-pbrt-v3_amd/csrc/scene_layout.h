// hprt — host half of scene creation: checks an HprtSceneDesc against what the kernels assume and lays out every per-scene
// array of the HBM scene (device/dev_scene.h).  No HIP runtime call: a malformed description is refused the same without a
// device.  hprt_scene_create (capi_device.hip) uploads the result.
#pragma once
#include <cstdint>
#include <vector>
#include "../../include/hprt.h"
#include "device/dev_scene.h"
#include "shadow_grid.h"
#include "distant_grid.h"

namespace hprt {

struct SceneLayout {
    // the arrays DevScene points at, as they are uploaded
    std::vector<DevPair> pairs;
    std::vector<DevWide> wide;                     // empty: the scene keeps the binary walk
    std::vector<float4> leafBox, tris, primN;
    std::vector<uint32_t> primVtx;
    std::vector<float> vUV, vS;
    std::vector<DevShape> shapes;
    std::vector<DevSphere> spheres;
    std::vector<DevMaterial> materials;
    std::vector<DevTexture> textures;
    std::vector<DevMipLevel> mipLevels;
    std::vector<float> texels, weightLut;
    std::vector<DevLight> lights;
    std::vector<DevEnvLight> envLights;
    std::vector<float> envData;
    std::vector<DevInstance> instances;
    std::vector<float4> topEntry, topEntryWide;    // empty without instances (topEntryWide: also without wide records)
    std::vector<float> lightFunc, lightCdf;
    // the scalars DevScene and HprtScene carry
    float funcInt = 0.f, worldRadius = 0.f;
    float wbMin[3] = {0, 0, 0}, wbMax[3] = {0, 0, 0};
    int lightStrategy = 0;                         // 0 uniform, 1 power, 2 spatial (voxN: its grid)
    int voxN[3] = {1, 1, 1};
    uint32_t nPrims = 0;                           // over all aggregates
    std::vector<uint32_t> topOrder;                // the top level's prim_order
    // per object definition: its prim_order and where its ordered primitives start in `tris` (a tree over an object's
    // creation-order primitives is mapped through them, as a top-level tree is through topOrder)
    std::vector<std::vector<uint32_t>> objectOrder;
    std::vector<uint32_t> objectPrimBase;
    std::vector<int32_t> instanceObject;           // per instance, its object definition
    bool instanced = false, hasSubstrateBin = false;
    // per ordered primitive: its leaf holds that one triangle alone, marked WIDE_LEAF_BOXED | WIDE_LEAF_FIRST in the wide records
    std::vector<uint8_t> primSingle;
    // the candidate grid of the shadow rays, for a triangle-only scene without instances that is lit by one light and takes the
    // leaf-exact walk: light-centred for a point light (shadow_grid.h), light-aligned for a distant light (distant_grid.h).
    // gridKind: which builder filled `grid` (None: neither was tried); grid.lists.eligible: the scene has that grid.  frame and
    // the margins are the distant grid's.
    GridKind gridKind = GridKind::None;
    DistantGrid grid;
    ShadowGridImage gridImage;                     // what is uploaded of it (filled when grid.lists.eligible)
};

// Validates *d and fills *out; HPRT_OK or an HPRT_E_* code with hprt_last_error() set.
int BuildSceneLayout(const HprtSceneDesc &d, SceneLayout *out);

// RadicalInverse(0..4, i), i < 128: SpatialLightDistribution's 128 sample points per voxel, as [5][128]
void VoxelSamplePoints(float *out);

}  // namespace hprt
