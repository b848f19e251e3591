// hprt — host RBSP builder: RBSP::buildTree (accelerators/rbsp.cpp:181-403) with the defaults of CreateRBSPTreeAccelerator
// (:549-571).  A restricted BSP tree is a kd-tree whose split planes may also be oblique: each interior node cuts along one of
// M = 3, 7, 9 or 13 fixed directions (getDirections, accelerators/RBSPShared.h), and the surface areas of the cost model are
// those of the node's k-DOP (kDOPMesh.h).  The output is the reference's, byte for byte: the 8-byte RBSPNode[] with its unions
// and flag packing, primitiveIndices, and onePrimitive in one-primitive leaves (primitives numbered in creation order).
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>
#include "bsp_tree.h"
#include "cost_hook.h"
#include "kdop_cost.h"

namespace hprt {

// RBSPNode (accelerators/rbsp.cpp:15-160), 8 bytes; off = 32 - clz(M) (2, 3, 4, 4 for M = 3, 7, 9, 13), mask = (1 << off) - 1:
//   a: interior split (float bits) | leaf onePrimitive (one primitive) | leaf primitiveIndicesOffset (more than one) | 0 (empty leaf)
//   b: interior axis | aboveChild << off;  leaf M | nPrimitives << off.  A node is a leaf iff (b & mask) == M.
using RbspNode = BspNode;                 // (bsp_tree.h)

// Deepest tree the device walk takes: pbrt's maxTodo (accelerators/rbsp.cpp:416).  A deeper tree is refused, never truncated.
enum : uint32_t { RBSP_TODO_MAX = 64u, RBSP_MAX_DIRECTIONS = 13u };

inline uint32_t RbspBitOffset(uint32_t M) { return 32u - (uint32_t)__builtin_clz(M); }   // getBitOffset: log2_fast(M + 1)
inline uint32_t RbspBitMask(uint32_t M) { return (1u << RbspBitOffset(M)) - 1u; }

// One node's candidates, as costFn sees them (kdop_cost.h: Edge is kdop::KEdge field for field, Cand the builder's candidate)
struct RbspCostRequest {
    const kdopcost::Edge *mesh; uint32_t nEdges;
    const float *dirs; uint32_t M;
    bool kdAware;
    kdopcost::Scalars sc;
    const kdopcost::Cand *cands; size_t n;
    float *costs, *costsFixed;            // costsFixed: NULL unless kdAware
    uint8_t *overflow;
};

// costFn, costMinCandidates, stats, costDone: the costing hook (cost_hook.h; the device-assisted build, hprt_rbsp_build_device)
struct RbspParams : CostHook<RbspCostRequest> {
    int isectCost = 80, travCost = 5;     // "intersectcost", "traversalcost"
    float emptyBonus = 0.f;               // "emptybonus"
    int maxPrims = 1, maxDepth = -1;      // "maxprims", "maxdepth" (-1: round(2 + 1.6 Log2Int(N)), core/geometry.h:1845)
    int nDirections = 3;                  // "nbDirections": 3, 7, 9 or 13
    int threads = 0;                      // candidate evaluation threads: 0 = OMP_NUM_THREADS (else 16), at most 16
    // RBSPKd::buildTree (accelerators/rbspKd.cpp:194-488, CreateRBSPKdTreeAccelerator :640-665): the kd-aware cost model.  Axis
    // candidates cost kdTravCost + C_isect; oblique ones BSP_ALPHA * isectCost * (N - 1) + kdTravCost + C_isect for the split
    // chosen, and travCost + C_isect for a second minimum that only the leaf tests read.
    bool kdAware = false;
    int kdTravCost = 1;                   // "kdtraversalcost"
};

struct RbspTree {
    std::vector<RbspNode> nodes;
    std::vector<uint32_t> primIndices;    // primitiveIndices
    std::vector<float> directions;        // 3 * M: getDirections(M)
    float bounds[6] = {0, 0, 0, 0, 0, 0}; // GenericBSP::bounds (the union of the primitives' world bounds): pMin, pMax
    uint32_t nPrims = 0, M = 3, leaves = 0, depth = 0, maxDepth = 0;   // depth: RBSPNode::depth of the root (interior levels)
};

// getDirections(M) (accelerators/RBSPShared.h): false for anything but 3, 7, 9 and 13
bool RbspDirections(uint32_t M, std::vector<float> *dirs3);

// One primitive per entry, in creation order.  isTri[i] != 0: tri9[9 i ..] holds the triangle's three world-space vertices
// (Triangle::getBounds, shapes/triangle.cpp:661-675); otherwise the projections are those of the 8 corners of the world bound
// (Shape::getBounds, core/shape.h:103-111).  bmin / bmax: Primitive::WorldBound() (the tree's root interval).
// Returns "" on success, else what went wrong (unsupported M, a tree outside the reference's primitive buffer).
std::string BuildRbspTree(size_t n, const float *bmin, const float *bmax, const float *tri9, const uint8_t *isTri, const RbspParams &p,
                          RbspTree *out);
// The candidates of rq costed with the vector code of kdop_mesh.h (Cut + SurfaceArea) and costRange's formulas, on the calling
// thread: what the diagnostics hook hprt_debug_kdop_cost calls impl 0.  overflow is cleared.
void RbspCostVector(const RbspCostRequest &rq);
// The interior nodes of a tree by kind: axis directions (kd, direction < 3) and oblique ones (bsp).
void RbspInteriorCounts(const RbspTree &t, uint32_t *kd, uint32_t *bsp);
// Structural check of a tree handed to the device: child offsets, leaf index ranges, primitive numbers, depth.
// Returns an empty string when the tree is well-formed, else what is wrong.
const char *CheckRbspTree(const RbspTree &t, uint32_t *depthOut);

}  // namespace hprt
