// hprt — library-internal glue shared by capi_host.cpp and capi_device.hip.
#pragma once
#include <string>
#include <vector>
#include "../../include/hprt.h"
#include "bvh_builder.h"
#include "kdtree_builder.h"
#include "rbsp_builder.h"
#include "bsppaper_builder.h"
#include "scene_model.h"

struct HprtModel { hprt::SceneModel sc; };
struct HprtBvh {
    hprt::BvhTree tree;                       // top-level aggregate (renderOptions->primitives)
    std::vector<hprt::BvhTree> objects;       // one per object definition (the accelerator ObjectInstance builds, core/api.cpp:1798-1806)
};

struct HprtKdTree { hprt::KdTree tree; };
// Two-level trees (pbrtObjectInstance, core/api.cpp:1794-1819): the top-level tree over the top-level items, and per object
// definition its own tree — none (no nodes) for an object of one primitive, which is wrapped as it is (:1798).  Tree: KdTree
// (HprtKdInst), RbspTree (HprtRbspInst), BspPaperTree (HprtBspPaperInst); what a further tree type has to supply: DESIGN.md §8k
template <typename Tree> struct HprtTwoLevel {
    Tree top;
    std::vector<Tree> objects;                // objects[o].nPrims: the object's primitives, tree (nodes) or not
    std::vector<int32_t> instanceObject;      // per instance, its object definition
};
struct HprtKdInst : HprtTwoLevel<hprt::KdTree> {};
struct HprtRbsp { hprt::RbspTree tree; };
struct HprtRbspKd { hprt::RbspTree tree; };     // built with RbspParams::kdAware
// Two-level RBSP trees (Accelerator "rbsp" / "rbspkd"): one handle type for both cost models; every tree is built with the same
// parameters, so all share M and the direction table.
struct HprtRbspInst : HprtTwoLevel<hprt::RbspTree> {
    bool kdAware = false;                     // built by hprt_rbspkdinst_build: walked with the kd form at axis nodes
};
struct HprtBspPaper { hprt::BspPaperTree tree; };
struct HprtBspPaperKd { hprt::BspPaperTree tree; };     // built with BspPaperParams::kdAware
// Two-level general BSP trees (Accelerator "bsppaper" / "bsppaperkd"): one handle type for both cost models and node layouts; every
// tree is built with the same parameters, so all carry BSPNode's flags or all BSPKdNode's.  The two-level node-based trees
// (hprt_bspnodeinst_build) are structurally these and use this handle: kd-aware for the fastkd form.
struct HprtBspPaperInst : HprtTwoLevel<hprt::BspPaperTree> {
    bool kdAware = false;                     // built by hprt_bsppaperkdinst_build or as a fastkd tree: BSPKdNode's flags, walked with the kd form at kd nodes
};

namespace hprt {
extern thread_local std::string g_lastError;
int SetError(int code, const std::string &msg);
int HandleException();      // maps the exception in flight to an HPRT_E_* code + message (capi_host.cpp)
// BuildSceneLayout (scene_layout.cpp) on *d, for hprt_debug_shape_inline: per ordered primitive the tag word and the word beside it (a
// triangle's or sphere's shape), per shape its DevShape flags and material
int LayoutTagsForDebug(const HprtSceneDesc &d, std::vector<uint32_t> *tags, std::vector<uint32_t> *primShape, std::vector<uint32_t> *shapeFlags,
                       std::vector<int32_t> *shapeMaterial);
// BuildSceneLayout on *d, for hprt_debug_shadow_grid_layout: out8 = {point grid: eligible, R; distant grid: eligible, R, entries, near-list
// length, bytes of the image, longest list}
int LayoutGridsForDebug(const HprtSceneDesc &d, double out8[8]);
}  // namespace hprt
