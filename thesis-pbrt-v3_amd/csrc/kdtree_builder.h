// hprt — host kd-tree builder: KdTreeAccel::buildTree (accelerators/kdtreeaccel.cpp:212-380) with the defaults of
// CreateKdTreeAccelerator (:523-545).  The output is the reference's, byte for byte: the 8-byte KdAccelNode[] with its unions
// and flag packing, primitiveIndices, and onePrimitive in one-primitive leaves (primitives numbered in creation order).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>
#include "bsp_tree.h"

namespace hprt {

// KdAccelNode (accelerators/kdtreeaccel.cpp:44-160), 8 bytes:
//   a: interior split (float bits) | leaf onePrimitive (one primitive) | leaf primitiveIndicesOffset (more than one) | 0 (empty leaf)
//   b: interior axis | aboveChild << 2;  leaf 3 | nPrimitives << 2
// (bsp_tree.h's node with M = 3)
using KdNode = BspNode;

// Deepest tree the device walk takes (its todo list holds at most the tree's depth): pbrt's maxTodo
// (accelerators/kdtreeaccel.cpp:393).  A deeper tree is refused, never truncated.
enum : uint32_t { KD_TODO_MAX = 64u };

struct KdParams {
    int isectCost = 80, travCost = 1;     // "intersectcost", "traversalcost"
    float emptyBonus = 0.f;               // "emptybonus"
    int maxPrims = 1, maxDepth = -1;      // "maxprims", "maxdepth" (-1: round(2 + 1.6 Log2Int(N)), core/geometry.h:1845)
};

struct KdTree {
    std::vector<KdNode> nodes;
    std::vector<uint32_t> primIndices;    // primitiveIndices
    float bounds[6] = {0, 0, 0, 0, 0, 0}; // KdTreeAccel::bounds: pMin, pMax
    uint32_t nPrims = 0, leaves = 0, depth = 0, maxDepth = 0;   // depth: KdAccelNode::depth of the root (interior levels)
};

// bmin / bmax: 3 floats per primitive in creation order (Primitive::WorldBound())
void BuildKdTree(size_t n, const float *bmin, const float *bmax, const KdParams &p, KdTree *out);
// Structural check of a tree handed to the device: child offsets, leaf index ranges, primitive numbers, depth.
// Returns an empty string when the tree is well-formed, else what is wrong.
const char *CheckKdTree(const KdTree &t, uint32_t *depthOut);

}  // namespace hprt
