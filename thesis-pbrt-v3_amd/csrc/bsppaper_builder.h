// hprt — host builder of the fork's general BSP tree (Accelerator "bsppaper"): BSPPaper::buildTree (accelerators/bspPaper.cpp:34-305)
// with the defaults of CreateBSPPaperTreeAccelerator (:308-319), after Ize, Wald and Parker, "Ray tracing with the BSP tree" (2008).
// Its split planes are the three axis planes through the primitives' world bounds and, per triangle, the triangle's own plane and
// the three planes through its edges that stand perpendicular to it (Triangle::getBSPPaperPlanes, shapes/triangle.cpp:678-720).  The
// surface areas of the cost model are those of the node's k-DOP, whose direction list grows along the path (KDOPMeshWithDirections,
// kDOPMesh.h:238-266); a plane candidate's primitive counts come from a BVH over the node's primitives (BVHAccel::
// getAmountToLeftAndRight, accelerators/bvh.cpp:439-470).  The output is the reference's, byte for byte: the 20-byte BSPNode[]
// (BSP.h:122-184) as an 8-byte GenericBSP node with M = 1 (bsp_tree.h) plus the node's 12-byte splitAxis, and primitiveIndices.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>
#include "bsp_cost.h"
#include "bsp_tree.h"
#include "cost_hook.h"

namespace hprt {

struct BvhNode;       // bvh_builder.h

// BSPNode's first 8 bytes: a = split (float bits) | onePrimitive | primitiveIndicesOffset; b = flags: leaf 1 | nPrims << 1, interior
// 0 | aboveChild << 1 (treeInitLeaf / treeInitInterior, BSP.h:11-35) — bsp_tree.h's node with M = 1 (off 1, mask 1).
enum : uint32_t { BSPPAPER_TODO_MAX = 64u, BSPPAPER_M = 1u, BSPPAPER_OFF = 1u, BSPPAPER_MASK = 1u };
// BSPKdNode's flags (BSPKd.h:11-57), the kd-aware tree's: the low 3 bits are 0-2 a kd interior node with that axis, 3 a leaf, 4 a
// plane interior node; aboveChild / nPrims << 3
enum : uint32_t { BSPPAPERKD_TODO_MAX = 64u, BSPPAPERKD_LEAF = 3u, BSPPAPERKD_PLANE = 4u, BSPPAPERKD_OFF = 3u, BSPPAPERKD_MASK = 7u };

// One node's candidates, as costFn sees them (bsp_cost.h: Edge is kdop::KEdge field for field, Cand the builder's candidate).  The
// axis candidates come first (nAxis of them), then the plane candidates.  bvhNodes / bvh: the BVH over the node's primitives as
// BuildBvh left it and as NodeBvh::side reads it (BspBvhRecords); both empty when no primitive has a plane.  primNums: the node's
// primitives; bmin .. isTri: the build's primitives (nTotal of them).
struct BspCostRequest {
    const kdopcost::Edge *mesh; uint32_t nEdges;          // face ids below 2 M
    const float *dirs; uint32_t M;                        // the node's own direction list
    bool kdAware;
    bspcost::Scalars sc;
    bspcost::Cand *cands; size_t n, nAxis;                // nBelow / nAbove of a costed plane candidate are written here
    const BvhNode *bvhNodes; const bspcost::BvhRec *bvh; uint32_t nBvh;
    const uint32_t *primOrder, *primNums; uint32_t nPrims;
    const float *bmin, *bmax, *tri9; const uint8_t *isTri; size_t nTotal;
    float *costs, *costsFixed;                            // costsFixed: NULL unless kdAware
    uint8_t *overflow;                                    // 1: not costed (a capacity of the costing was exceeded)
    uint32_t level;                                       // the node's depth below the root (diagnostics)
};

// costFn, costMinCandidates, stats, costDone: the costing hook (cost_hook.h; the device-assisted build, hprt_bsppaper_build_device).
// Besides the costs, costFn fills nBelow / nAbove of every plane candidate it has costed.
struct BspPaperParams : CostHook<BspCostRequest> {
    int isectCost = 80, travCost = 5;     // "intersectcost", "traversalcost"
    float emptyBonus = 0.f;               // "emptybonus"
    int maxPrims = 1, maxDepth = -1;      // "maxprims", "maxdepth" (-1: round(2 + 1.6 Log2Int(N)), core/geometry.h:1845)
    int threads = 0;                      // candidate evaluation threads: 0 = OMP_NUM_THREADS (else 16), at most 16
    // Accelerator "bsppaperkd": BSPPaperKd::buildTree (accelerators/bspPaperKd.cpp:34-339) with the defaults of
    // CreateBSPPaperKdTreeAccelerator (:341-353).  Axis candidates cost kdTravCost + C_isect, plane candidates
    // 0.1f * isectCost * (N - 1) + kdTravCost + C_isect; a second minimum, travCost + C_isect over the plane candidates, takes part in
    // the leaf tests and supplies the split only where the first is unset; nodes carry BSPKdNode's flags (BSPPAPERKD_*)
    bool kdAware = false;
    int kdTravCost = 1;                   // "kdtraversalcost"
};

struct BspPaperTree {
    std::vector<BspNode> nodes;
    std::vector<float> axes;              // 3 per node: splitAxis of interior nodes, zero for leaves (the reference leaves them unset)
    std::vector<uint32_t> primIndices;    // primitiveIndices
    float bounds[6] = {0, 0, 0, 0, 0, 0}; // GenericBSP::bounds (the union of the primitives' world bounds): pMin, pMax
    uint32_t nPrims = 0, leaves = 0, depth = 0, maxDepth = 0;   // depth: interior levels of the deepest path
    uint32_t axisNodes = 0, planeNodes = 0;                     // interior nodes of the axis sweep (nbKdNodes) / of a triangle's plane (nbBSPNodes)
    bool kdAware = false;                                       // nodes hold BSPKdNode's flags; axes of kd nodes are zero like the leaves'
};

// One candidate plane of a primitive: Plane {t, axis} (core/geometry.h:1864-1868)
struct BspPlane { float t, axis[3]; };
// Triangle::getBSPPaperPlanes over the triangle p0 p1 p2 (9 floats): up to four planes, none for a degenerate triangle
std::vector<BspPlane> BspPaperTrianglePlanes(const float *p9);

// A BVH over a node's primitives (bvh_builder.h, isectCost 4, travCost 8, maxPrims 1) and the two classifications the build makes
// over it: BVHAccel::getAmountToLeftAndRight (counts) and getPrimnumsToLeftAndRight (the local primitive numbers, in the order its
// stack visits them).  n primitives with world bounds bmin / bmax (3 floats each); isTri[i] != 0: tri9[9 i ..] holds the
// triangle's vertices (Triangle::getBounds), else a primitive projects its world bound's corners (Shape::getBounds).  Exposed for
// the tests (hprt_debug_bsppaper_classify).
void BspPaperClassify(size_t n, const float *bmin, const float *bmax, const float *tri9, const uint8_t *isTri, const BspPlane &plane,
                      uint32_t counts[2], std::vector<uint32_t> *left, std::vector<uint32_t> *right);

// One primitive per entry, in creation order (as BuildRbspTree).  Returns "" on success, else what went wrong (a tree outside the
// reference's (maxDepth + 1) * N primitive buffer).
std::string BuildBspPaperTree(size_t n, const float *bmin, const float *bmax, const float *tri9, const uint8_t *isTri, const BspPaperParams &p,
                              BspPaperTree *out);
// What NodeBvh::side computes from a BVH node's box, with its operations: the centre and half the diagonal's length (out: n records)
void BspBvhRecords(const BvhNode *nodes, size_t n, bspcost::BvhRec *out);
// The candidates of rq costed with the builder's own code (CutMeasure over the vector meshes, NodeBvh::count over bvhNodes) and
// costRange's formulas, on the calling thread: what the diagnostics hook hprt_debug_bsp_cost calls impl 0.  overflow is cleared.
void BspCostVector(const BspCostRequest &rq);
// Structural check of a tree handed to the device: CheckBspNodes with M = 1, one axis per node, every interior axis finite and
// non-zero.  Returns an empty string when the tree is well-formed, else what is wrong.
const char *CheckBspPaperTree(const BspPaperTree &t, uint32_t *depthOut);
// The same for a kd-aware tree: every node's kind is 0-4, child offsets and leaf ranges as CheckBspNodes with 3 flag bits, and
// every plane node's axis finite and non-zero.
const char *CheckBspPaperKdTree(const BspPaperTree &t, uint32_t *depthOut);

}  // namespace hprt
