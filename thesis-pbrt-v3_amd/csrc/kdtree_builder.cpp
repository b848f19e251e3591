// hprt — KdTreeAccel::buildTree (accelerators/kdtreeaccel.cpp:212-380), restated operation for operation.
#include "kdtree_builder.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

namespace hprt {
namespace {

struct Box { float lo[3], hi[3]; };
// Bounds3::SurfaceArea (core/geometry.h): 2 * (d.x * d.y + d.x * d.z + d.y * d.z)
inline float SurfaceArea(const Box &b) {
    const float dx = b.hi[0] - b.lo[0], dy = b.hi[1] - b.lo[1], dz = b.hi[2] - b.lo[2];
    return 2 * (dx * dy + dx * dz + dy * dz);
}
inline float fmin_std(float a, float b) { return (b < a) ? b : a; }   // std::min
inline float fmax_std(float a, float b) { return (a < b) ? b : a; }   // std::max

enum class EdgeType : int { Start, End };
struct BoundEdge { float t; uint32_t primNum; EdgeType type; };     // accelerators/genericBSP.h:47-60
struct BuildNode {                                                  // KdBuildNode, accelerators/kdtreeaccel.h:77-90
    uint32_t depth, nPrimitives, badRefines; Box nodeBounds; size_t primNums; uint32_t parentNum;     // primNums: offset into `prims`
};

// Log2Int(int64_t) (core/pbrt.h:345-362): 63 - clz
inline int Log2Int64(uint64_t v) { return v ? 63 - __builtin_clzll(v) : -1; }

}  // namespace

void BuildKdTree(size_t n, const float *bmin, const float *bmax, const KdParams &p, KdTree *out) {
    // CreateKdTreeAccelerator / GenericBSP: the parameters as the reference holds them (uint32_t, Float)
    const uint32_t isectCost = (uint32_t)p.isectCost, traversalCost = (uint32_t)p.travCost, maxPrims = (uint32_t)p.maxPrims;
    const float emptyBonus = p.emptyBonus;
    uint32_t maxDepth = (uint32_t)p.maxDepth;
    if (maxDepth == (uint32_t)-1) maxDepth = (uint32_t)std::round(2 + 1.6f * (float)Log2Int64((uint64_t)n));   // calculateMaxDepth
    KdTree &t = *out;
    t = KdTree();
    t.nPrims = (uint32_t)n;
    t.maxDepth = maxDepth;

    // bounds = Union of every primitive's WorldBound, from the empty Bounds3f
    Box bounds;
    for (int k = 0; k < 3; ++k) { bounds.lo[k] = std::numeric_limits<float>::max(); bounds.hi[k] = std::numeric_limits<float>::lowest(); }
    std::vector<Box> allPrimBounds(n);
    for (size_t i = 0; i < n; ++i) {
        Box &b = allPrimBounds[i];
        for (int k = 0; k < 3; ++k) {
            b.lo[k] = bmin[3 * i + k]; b.hi[k] = bmax[3 * i + k];
            bounds.lo[k] = fmin_std(bounds.lo[k], b.lo[k]); bounds.hi[k] = fmax_std(bounds.hi[k], b.hi[k]);
        }
    }
    for (int k = 0; k < 3; ++k) { t.bounds[k] = bounds.lo[k]; t.bounds[3 + k] = bounds.hi[k]; }

    std::vector<BoundEdge> edges[3];
    for (auto &e : edges) e.resize(2 * n);
    // the reference allocates (maxDepth + 1) * N entries up front; here the buffer grows to what the build reaches
    std::vector<uint32_t> prims(n + 1);
    for (size_t i = 0; i < n; ++i) prims[i] = (uint32_t)i;

    std::vector<KdNode> &nodes = t.nodes;
    auto initLeaf = [&](const uint32_t *primNums, uint32_t np) {     // KdAccelNode::InitLeaf (:187-200)
        KdNode nd;
        nd.b = 3u | (np << 2u);
        if (np == 0) nd.a = 0u;
        else if (np == 1) nd.a = primNums[0];
        else {
            nd.a = (uint32_t)t.primIndices.size();
            for (uint32_t i = 0; i < np; ++i) t.primIndices.push_back(primNums[i]);
        }
        nodes.push_back(nd);
        ++t.leaves;
    };

    uint32_t nodeNum = 0;
    std::vector<BuildNode> stack;
    stack.push_back(BuildNode{maxDepth, (uint32_t)n, 0u, bounds, 0, (uint32_t)-1});
    while (!stack.empty()) {
        BuildNode cur = stack.back();
        stack.pop_back();
        if (cur.parentNum != (uint32_t)-1) nodes[cur.parentNum].b |= (nodeNum << 2u);      // setAboveChild

        const uint32_t *primNums = &prims[cur.primNums];
        if (cur.nPrimitives <= maxPrims || cur.depth == 0) { initLeaf(primNums, cur.nPrimitives); ++nodeNum; continue; }

        // Choose split axis position for interior node
        uint32_t bestAxis = (uint32_t)-1, bestOffset = (uint32_t)-1;
        float bestCost = std::numeric_limits<float>::infinity();
        const float oldCost = (float)isectCost * float(cur.nPrimitives);
        const float totalSA = SurfaceArea(cur.nodeBounds);
        const float invTotalSA = 1 / totalSA;
        float d[3];
        for (int k = 0; k < 3; ++k) d[k] = cur.nodeBounds.hi[k] - cur.nodeBounds.lo[k];
        for (uint32_t axis = 0; axis < 3; ++axis) {
            BoundEdge *e = edges[axis].data();
            for (uint32_t i = 0; i < cur.nPrimitives; ++i) {
                const uint32_t pn = primNums[i];
                const Box &b = allPrimBounds[pn];
                e[2 * i] = BoundEdge{b.lo[axis], pn, EdgeType::Start};
                e[2 * i + 1] = BoundEdge{b.hi[axis], pn, EdgeType::End};
            }
            std::sort(e, e + 2 * cur.nPrimitives, [](const BoundEdge &e0, const BoundEdge &e1) -> bool {
                if (e0.t == e1.t) return (int)e0.type < (int)e1.type;
                else return e0.t < e1.t;
            });
            uint32_t nBelow = 0, nAbove = cur.nPrimitives;
            for (uint32_t i = 0; i < 2 * cur.nPrimitives; ++i) {
                if (e[i].type == EdgeType::End) --nAbove;
                const float edgeT = e[i].t;
                if (edgeT > cur.nodeBounds.lo[axis] && edgeT < cur.nodeBounds.hi[axis]) {
                    const uint32_t otherAxis0 = (axis + 1) % 3, otherAxis1 = (axis + 2) % 3;
                    const float belowSA = 2 * (d[otherAxis0] * d[otherAxis1] + (edgeT - cur.nodeBounds.lo[axis]) * (d[otherAxis0] + d[otherAxis1]));
                    const float aboveSA = 2 * (d[otherAxis0] * d[otherAxis1] + (cur.nodeBounds.hi[axis] - edgeT) * (d[otherAxis0] + d[otherAxis1]));
                    const float pBelow = belowSA * invTotalSA;
                    const float pAbove = aboveSA * invTotalSA;
                    const float eb = (nAbove == 0 || nBelow == 0) ? emptyBonus : 0;
                    const float cost = (float)traversalCost + (float)isectCost * (1 - eb) * (pBelow * (float)nBelow + pAbove * (float)nAbove);
                    if (cost < bestCost) { bestCost = cost; bestAxis = axis; bestOffset = i; }
                }
                if (e[i].type == EdgeType::Start) ++nBelow;
            }
        }

        // Create leaf if no good splits were found
        if (bestCost > oldCost) ++cur.badRefines;
        if ((bestCost > 4 * oldCost && cur.nPrimitives < 16) || bestAxis == (uint32_t)-1 || cur.badRefines == 3) {
            initLeaf(primNums, cur.nPrimitives); ++nodeNum; continue;
        }

        // Classify primitives with respect to split: prims1 first, in place, so that child 0's share does not overwrite it
        const BoundEdge *e = edges[bestAxis].data();
        uint32_t n0 = 0, n1 = 0;
        const size_t prims1 = cur.primNums;
        for (uint32_t i = bestOffset + 1; i < 2 * cur.nPrimitives; ++i)
            if (e[i].type == EdgeType::End) prims[prims1 + n1++] = e[i].primNum;
        const size_t prims0 = prims1 + n1;
        if (prims.size() < prims0 + cur.nPrimitives) prims.resize(prims0 + cur.nPrimitives);
        for (uint32_t i = 0; i < bestOffset; ++i)
            if (e[i].type == EdgeType::Start) prims[prims0 + n0++] = e[i].primNum;

        const float tSplit = e[bestOffset].t;
        Box bounds0 = cur.nodeBounds, bounds1 = cur.nodeBounds;
        bounds0.hi[bestAxis] = bounds1.lo[bestAxis] = tSplit;
        KdNode nd;                                     // InitInterior
        std::memcpy(&nd.a, &tSplit, 4);
        nd.b = bestAxis;
        nodes.push_back(nd);
        stack.push_back(BuildNode{cur.depth - 1, n1, cur.badRefines, bounds1, prims1, nodeNum});
        stack.push_back(BuildNode{cur.depth - 1, n0, cur.badRefines, bounds0, prims0, (uint32_t)-1});
        ++nodeNum;
    }
    uint32_t depth = 0;
    (void)CheckKdTree(t, &depth);
    t.depth = depth;
}

const char *CheckKdTree(const KdTree &t, uint32_t *depthOut) {
    return CheckBspNodes(t.nodes, t.primIndices, t.nPrims, 3u, 2u, 3u, depthOut);      // KdAccelNode: M = 3 (bsp_tree.h)
}

}  // namespace hprt
