// hprt — RBSP::buildTree (accelerators/rbsp.cpp:181-403) and RBSPKd::buildTree (accelerators/rbspKd.cpp:194-488,
// RbspParams::kdAware) with KDOPCut / KDOPSurfaceArea (accelerators/kDOPMesh.h), restated operation for operation.  Every float
// operation is one IEEE rounding in the reference's order (built with -ffp-contract=off).
//
// The one liberty: the candidates of a node may be costed on several threads.  Each candidate's cost is a pure function of the
// node's k-DOP and the candidate, and the reduction keeps the first minimum in (direction, edge) order — what the reference's
// strict `cost < bestCost` scan keeps (for RBSPKd, each of its two minima) — so the tree does not depend on the thread count.
// The winner's two halves are then cut and measured once more, exactly as the scan left them.
#include "rbsp_builder.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <thread>
#include "kdop_mesh.h"

namespace hprt {
namespace {

using namespace kdop;

enum class EdgeType : int { Start, End };
struct BoundEdge { float t; uint32_t primNum; EdgeType type; };     // accelerators/genericBSP.h:47-58
struct Range { float min, max; };                                   // Bounds<Float>
struct BuildNode {                                                  // RBSPBuildNode, accelerators/RBSPShared.h:11-27
    uint32_t depth, nPrimitives, badRefines;
    std::vector<Range> nodeBounds;
    Mesh mesh; float meshArea;
    size_t primNums; uint32_t parentNum;                            // primNums: offset into `prims`
};
using Cand = kdopcost::Cand;                                       // {d, i, nBelow, nAbove, t}
static_assert(sizeof(KEdge) == sizeof(kdopcost::Edge) && sizeof(KEdge) == 32, "kdop_cost.h restates KEdge");

// Log2Int(int64_t) (core/pbrt.h:345-362): 63 - clz
inline int Log2Int64(uint64_t v) { return v ? 63 - __builtin_clzll(v) : -1; }


}  // namespace

bool RbspDirections(uint32_t M, std::vector<float> *out) {
    if (M != 3 && M != 7 && M != 9 && M != 13) return false;
    std::vector<float> &d = *out;
    d.clear();
    auto add = [&](float x, float y, float z) { d.push_back(x); d.push_back(y); d.push_back(z); };
    auto addNormalized = [&](float x, float y, float z) {
        // Normalize(v) = v / v.Length() and Vector3::operator/ multiplies by (Float)1 / f
        const float len = std::sqrt(x * x + y * y + z * z);
        const float inv = (float)1 / len;
        add(x * inv, y * inv, z * inv);
    };
    add(1.f, 0.f, 0.f); add(0.f, 1.f, 0.f); add(0.f, 0.f, 1.f);
    if (M == 7 || M == 13) {
        addNormalized(1.f, 1.f, 1.f); addNormalized(1.f, -1.f, 1.f); addNormalized(1.f, 1.f, -1.f); addNormalized(1.f, -1.f, -1.f);
    }
    if (M == 9 || M == 13) {
        addNormalized(1.f, 1.f, 0.f); addNormalized(1.f, 0.f, 1.f); addNormalized(0.f, 1.f, 1.f);
        addNormalized(1.f, -1.f, 0.f); addNormalized(1.f, 0.f, -1.f); addNormalized(0.f, 1.f, -1.f);
    }
    return true;
}

std::string BuildRbspTree(size_t n, const float *bmin, const float *bmax, const float *tri9, const uint8_t *isTri, const RbspParams &p,
                          RbspTree *out) {
    RbspTree &t = *out;
    t = RbspTree();
    const uint32_t M = (uint32_t)p.nDirections;
    if (p.nDirections <= 0 || !RbspDirections(M, &t.directions))
        return "nbDirections " + std::to_string(p.nDirections) + " is not supported (3, 7, 9 or 13)";
    const float *dirs = t.directions.data();
    const uint32_t off = RbspBitOffset(M);
    // CreateRBSPTreeAccelerator / GenericBSP: the parameters as the reference holds them (uint32_t, Float)
    const uint32_t isectCost = (uint32_t)p.isectCost, traversalCost = (uint32_t)p.travCost, maxPrims = (uint32_t)p.maxPrims;
    const float emptyBonus = p.emptyBonus;
    uint32_t maxDepth = (uint32_t)p.maxDepth;
    if (maxDepth == (uint32_t)-1) maxDepth = (uint32_t)std::round(2 + 1.6f * (float)Log2Int64((uint64_t)n));   // calculateMaxDepth
    t.nPrims = (uint32_t)n; t.M = M; t.maxDepth = maxDepth;
    const int nThreads = ThreadCount(p.threads);

    // bounds = Union of every WorldBound; per-direction root bounds = Union of the primitives' projections (getBounds)
    float lo[3], hi[3];
    for (int k = 0; k < 3; ++k) { lo[k] = std::numeric_limits<float>::max(); hi[k] = std::numeric_limits<float>::lowest(); }
    std::vector<Range> root(M, Range{std::numeric_limits<float>::max(), std::numeric_limits<float>::lowest()});
    std::vector<Range> allPrimBounds((size_t)n * M);
    for (size_t i = 0; i < n; ++i) {
        for (int k = 0; k < 3; ++k) { lo[k] = fmin_std(lo[k], bmin[3 * i + k]); hi[k] = fmax_std(hi[k], bmax[3 * i + k]); }
        for (uint32_t d = 0; d < M; ++d) {
            const float *dir = dirs + 3 * d;
            Range b;
            if (isTri[i]) {     // Triangle::getBounds
                const float *v = tri9 + 9 * i;
                float tt = Dot(dir, P3{v[0], v[1], v[2]});
                float mn = tt, mx = tt;
                for (int c = 1; c < 3; ++c) {
                    tt = Dot(dir, P3{v[3 * c], v[3 * c + 1], v[3 * c + 2]});
                    if (tt > mx) mx = tt;
                    else if (tt < mn) mn = tt;
                }
                b = Range{mn, mx};
            } else {            // Shape::getBounds: the 8 corners of WorldBound (Bounds3::Corner)
                b = Range{std::numeric_limits<float>::max(), std::numeric_limits<float>::lowest()};
                const float *bl = bmin + 3 * i, *bh = bmax + 3 * i;
                for (int c = 0; c < 8; ++c) {
                    const P3 q{(c & 1) ? bh[0] : bl[0], (c & 2) ? bh[1] : bl[1], (c & 4) ? bh[2] : bl[2]};
                    const float proj = Dot(dir, q);
                    if (proj < b.min) b.min = proj;
                    if (proj > b.max) b.max = proj;
                }
            }
            allPrimBounds[i * M + d] = b;
            root[d] = Range{fmin_std(root[d].min, b.min), fmax_std(root[d].max, b.max)};
        }
    }
    for (int k = 0; k < 3; ++k) { t.bounds[k] = lo[k]; t.bounds[3 + k] = hi[k]; }

    // Bounds3::toKDOPMesh (core/geometry.h:1001-1027): the 12 edges of the box with their face ids
    Mesh rootMesh;
    {
        const P3 v1{lo[0], lo[1], lo[2]}, v2{lo[0], lo[1], hi[2]}, v3{lo[0], hi[1], lo[2]}, v4{hi[0], lo[1], lo[2]};
        const P3 v5{lo[0], hi[1], hi[2]}, v6{hi[0], lo[1], hi[2]}, v7{hi[0], hi[1], lo[2]}, v8{hi[0], hi[1], hi[2]};
        rootMesh = {{v1, v2, 1, 3}, {v1, v3, 1, 5}, {v1, v4, 3, 5}, {v2, v5, 1, 4}, {v2, v6, 3, 4}, {v3, v5, 1, 2},
                    {v3, v7, 2, 5}, {v4, v6, 0, 3}, {v4, v7, 0, 5}, {v5, v8, 2, 4}, {v6, v8, 0, 4}, {v7, v8, 0, 2}};
    }
    std::vector<Scratch> scratch((size_t)nThreads);
    const float rootArea = SurfaceArea(rootMesh, dirs, M, scratch[0]);    // evaluated before the mesh is stored

    std::vector<std::vector<BoundEdge>> edges(M);
    for (auto &e : edges) e.resize(2 * n);
    // the reference's primitive buffer: (maxDepth + 1) * N entries, written without a check; here a write past it is an error
    const uint64_t primsCap = ((uint64_t)maxDepth + 1) * (uint64_t)n;
    std::vector<uint32_t> prims(n + 1);
    for (size_t i = 0; i < n; ++i) prims[i] = (uint32_t)i;

    std::vector<RbspNode> &nodes = t.nodes;
    auto initLeaf = [&](const uint32_t *primNums, uint32_t np) {     // RBSPNode::InitLeaf (:163-177)
        RbspNode nd;
        nd.b = M | (np << off);
        if (np == 0) nd.a = 0u;
        else if (np == 1) nd.a = primNums[0];
        else {
            nd.a = (uint32_t)t.primIndices.size();
            for (uint32_t i = 0; i < np; ++i) t.primIndices.push_back(primNums[i]);
        }
        nodes.push_back(nd);
        ++t.leaves;
    };

    std::vector<Cand> cands;
    std::vector<uint8_t> overflow;              // per candidate: the costing hook could not cost it (RbspParams::costFn)
    std::vector<float> costs, costsFixed;       // costsFixed: RBSPKd's traversalCost + C_isect of the oblique candidates
    const float BSP_ALPHA = 0.1;                 // RBSPKd::buildTree's `const Float`
    const uint32_t kdTraversalCost = (uint32_t)p.kdTravCost;
    std::vector<std::thread> pool;
    uint32_t nodeNum = 0;
    std::vector<BuildNode> stack;
    stack.push_back(BuildNode{maxDepth, (uint32_t)n, 0u, root, rootMesh, rootArea, 0, (uint32_t)-1});
    while (!stack.empty()) {
        BuildNode cur = std::move(stack.back());
        stack.pop_back();
        if (cur.parentNum != (uint32_t)-1) nodes[cur.parentNum].b |= (nodeNum << off);      // setAboveChild

        if (cur.nPrimitives <= maxPrims || cur.depth == 0) { initLeaf(&prims[cur.primNums], cur.nPrimitives); ++nodeNum; continue; }

        const float oldCost = (float)isectCost * float(cur.nPrimitives);
        const float invTotalSA = 1 / cur.meshArea;
        // every candidate of every direction, in the reference's scan order
        cands.clear();
        for (uint32_t d = 0; d < M; ++d) {
            BoundEdge *e = edges[d].data();
            const uint32_t *primNums = &prims[cur.primNums];
            for (uint32_t i = 0; i < cur.nPrimitives; ++i) {
                const uint32_t pn = primNums[i];
                const Range &b = allPrimBounds[(size_t)pn * M + d];
                e[2 * i] = BoundEdge{b.min, pn, EdgeType::Start};
                e[2 * i + 1] = BoundEdge{b.max, pn, EdgeType::End};
            }
            std::sort(e, e + 2 * cur.nPrimitives, [](const BoundEdge &e0, const BoundEdge &e1) -> bool {
                if (e0.t == e1.t) return (int)e0.type < (int)e1.type;
                else return e0.t < e1.t;
            });
            uint32_t nBelow = 0, nAbove = cur.nPrimitives;
            for (uint32_t i = 0; i < 2 * cur.nPrimitives; ++i) {
                if (e[i].type == EdgeType::End) --nAbove;
                const float edgeT = e[i].t;
                if (edgeT > cur.nodeBounds[d].min && edgeT < cur.nodeBounds[d].max) cands.push_back(Cand{d, i, nBelow, nAbove, edgeT});
                if (e[i].type == EdgeType::Start) ++nBelow;
            }
        }
        costs.resize(cands.size());
        if (p.kdAware) costsFixed.resize(cands.size());
        auto costRange = [&](size_t k0, size_t k1, Scratch &s) {
            for (size_t k = k0; k < k1; ++k) {
                const Cand &c = cands[k];
                Cut(cur.mesh, M, c.t, dirs + 3 * c.d, c.d, s);
                const float areaBelow = SurfaceArea(s.left, dirs, M, s);
                const float areaAbove = SurfaceArea(s.right, dirs, M, s);
                const float pBelow = areaBelow * invTotalSA;
                const float pAbove = areaAbove * invTotalSA;
                const float eb = (c.nAbove == 0 || c.nBelow == 0) ? emptyBonus : 0;
                if (!p.kdAware) {
                    costs[k] = (float)traversalCost + (float)isectCost * (1 - eb) * (pBelow * (float)c.nBelow + pAbove * (float)c.nAbove);
                } else if (c.d < 3) {
                    costs[k] = (float)kdTraversalCost + (float)isectCost * (1 - eb) * (pBelow * (float)c.nBelow + pAbove * (float)c.nAbove);
                } else {
                    const float costIntersection = (float)isectCost * (1 - eb) * (pBelow * (float)c.nBelow + pAbove * (float)c.nAbove);
                    costsFixed[k] = (float)traversalCost + costIntersection;
                    costs[k] = BSP_ALPHA * (float)isectCost * (float)(cur.nPrimitives - 1) + (float)kdTraversalCost + costIntersection;
                }
            }
        };
        // the costing hook (RbspParams::costFn): the node's candidates costed elsewhere, the flagged ones repaired here
        std::string hookErr;
        const HookResult hooked = RunCostHook(p, cands.size(), overflow, true, [&](RbspCostRequest &rq) {
            rq.mesh = reinterpret_cast<const kdopcost::Edge *>(cur.mesh.data()); rq.nEdges = (uint32_t)cur.mesh.size();
            rq.dirs = dirs; rq.M = M; rq.kdAware = p.kdAware;
            rq.sc = kdopcost::Scalars{invTotalSA, emptyBonus, isectCost, traversalCost, kdTraversalCost, cur.nPrimitives, 0u};
            rq.cands = cands.data(); rq.n = cands.size();
            rq.costs = costs.data(); rq.costsFixed = p.kdAware ? costsFixed.data() : nullptr; rq.overflow = overflow.data();
        }, [&](size_t k) { costRange(k, k + 1, scratch[0]); }, &hookErr);
        if (hooked == HookResult::Failed) return hookErr;
        if (hooked == HookResult::Costed) {
            // (costs[] is complete)
        } else if (nThreads > 1 && cands.size() >= kParallelCandidates) {
            const size_t chunk = (cands.size() + nThreads - 1) / nThreads;
            pool.clear();
            for (int w = 1; w < nThreads; ++w) {
                const size_t k0 = std::min(cands.size(), w * chunk), k1 = std::min(cands.size(), (w + 1) * chunk);
                pool.emplace_back(costRange, k0, k1, std::ref(scratch[(size_t)w]));
            }
            costRange(0, std::min(cands.size(), chunk), scratch[0]);
            for (auto &th : pool) th.join();
        } else costRange(0, cands.size(), scratch[0]);
        // the reference's scan: strict `<`, so the first minimum in (direction, edge) order
        uint32_t bestD = (uint32_t)-1, bestOffset = (uint32_t)-1;
        float bestCost = std::numeric_limits<float>::infinity();
        for (size_t k = 0; k < cands.size(); ++k)
            if (costs[k] < bestCost) { bestCost = costs[k]; bestD = cands[k].d; bestOffset = cands[k].i; }

        if (p.kdAware) {
            // RBSPKd keeps a second minimum over the oblique candidates (costFixed); the leaf tests need both to fail
            uint32_t bestDFixed = (uint32_t)-1;
            float bestCostFixed = std::numeric_limits<float>::infinity();
            for (size_t k = 0; k < cands.size(); ++k)
                if (cands[k].d >= 3 && costsFixed[k] < bestCostFixed) { bestCostFixed = costsFixed[k]; bestDFixed = cands[k].d; }
            if (bestCost > oldCost && bestCostFixed > oldCost) ++cur.badRefines;
            if ((bestCost > 4 * oldCost && bestCostFixed > 4 * oldCost && cur.nPrimitives < 16) || (bestD == (uint32_t)-1 && bestDFixed == (uint32_t)-1) ||
                cur.badRefines == 3) {
                initLeaf(&prims[cur.primNums], cur.nPrimitives); ++nodeNum; continue;
            }
            // only the fixed minimum beat infinity: the reference classifies by edges[bestD = -1] (rbspKd.cpp:423-432)
            if (bestD == (uint32_t)-1)
                return "every kd-aware candidate cost is infinite or NaN while a fixed-cost oblique split exists: the reference's build is undefined there";
        } else {
            // Create leaf if no good splits were found
            if (bestCost > oldCost) ++cur.badRefines;
            if ((bestCost > 4 * oldCost && cur.nPrimitives < 16) || bestD == (uint32_t)-1 || cur.badRefines == 3) {
                initLeaf(&prims[cur.primNums], cur.nPrimitives); ++nodeNum; continue;
            }
        }

        // the winner's halves, measured (and so reoriented) as the scan left them
        const BoundEdge *e = edges[bestD].data();
        const float tSplit = e[bestOffset].t;
        Scratch &s = scratch[0];
        Cut(cur.mesh, M, tSplit, dirs + 3 * bestD, bestD, s);
        Mesh below = s.left, above = s.right;
        const float areaBelow = SurfaceArea(below, dirs, M, s);
        const float areaAbove = SurfaceArea(above, dirs, M, s);

        // Classify primitives with respect to split: prims1 first, in place, so that child 0's share does not overwrite it
        uint32_t n0 = 0, n1 = 0;
        const size_t prims1 = cur.primNums;
        for (uint32_t i = bestOffset + 1; i < 2 * cur.nPrimitives; ++i)
            if (e[i].type == EdgeType::End) prims[prims1 + n1++] = e[i].primNum;
        const size_t prims0 = prims1 + n1;
        uint32_t nStart = 0;
        for (uint32_t i = 0; i < bestOffset; ++i) nStart += e[i].type == EdgeType::Start;
        if ((uint64_t)prims0 + nStart > primsCap)
            return "the build needs more than the reference's (maxDepth + 1) * N primitive slots; lower \"maxdepth\"";
        if (prims.size() < prims0 + nStart + 1) prims.resize(prims0 + nStart + 1);
        for (uint32_t i = 0; i < bestOffset; ++i)
            if (e[i].type == EdgeType::Start) prims[prims0 + n0++] = e[i].primNum;

        // the children's per-direction bounds: the projections of their k-DOP edges (KDOPEdge::getBounds)
        std::vector<Range> bounds0(M, Range{std::numeric_limits<float>::max(), std::numeric_limits<float>::lowest()}), bounds1 = bounds0;
        for (uint32_t d = 0; d < M; ++d) {
            const float *dir = dirs + 3 * d;
            for (const KEdge &ke : below) {
                const float t1 = Dot(dir, ke.v1), t2 = Dot(dir, ke.v2);
                bounds0[d] = Range{fmin_std(bounds0[d].min, fmin_std(t1, t2)), fmax_std(bounds0[d].max, fmax_std(t1, t2))};
            }
            for (const KEdge &ke : above) {
                const float t1 = Dot(dir, ke.v1), t2 = Dot(dir, ke.v2);
                bounds1[d] = Range{fmin_std(bounds1[d].min, fmin_std(t1, t2)), fmax_std(bounds1[d].max, fmax_std(t1, t2))};
            }
        }
        RbspNode nd;                                   // InitInterior
        std::memcpy(&nd.a, &tSplit, 4);
        nd.b = bestD;
        nodes.push_back(nd);
        stack.push_back(BuildNode{cur.depth - 1, n1, cur.badRefines, std::move(bounds1), std::move(above), areaAbove, prims1, nodeNum});
        stack.push_back(BuildNode{cur.depth - 1, n0, cur.badRefines, std::move(bounds0), std::move(below), areaBelow, prims0, (uint32_t)-1});
        ++nodeNum;
    }
    uint32_t depth = 0;
    (void)CheckRbspTree(t, &depth);
    t.depth = depth;
    return "";
}

void RbspCostVector(const RbspCostRequest &rq) {
    // costRange of BuildRbspTree over a caller's mesh: the same calls and the same formulas, in the same order
    Mesh mesh(rq.nEdges);
    if (rq.nEdges) std::memcpy(static_cast<void *>(mesh.data()), rq.mesh, (size_t)rq.nEdges * sizeof(KEdge));
    Scratch s;
    const uint32_t M = rq.M, isectCost = rq.sc.isectCost, traversalCost = rq.sc.traversalCost, kdTraversalCost = rq.sc.kdTraversalCost;
    const float invTotalSA = rq.sc.invTotalSA, emptyBonus = rq.sc.emptyBonus;
    const float BSP_ALPHA = 0.1;
    for (size_t k = 0; k < rq.n; ++k) {
        const Cand &c = rq.cands[k];
        Cut(mesh, M, c.t, rq.dirs + 3 * c.d, c.d, s);
        const float areaBelow = SurfaceArea(s.left, rq.dirs, M, s);
        const float areaAbove = SurfaceArea(s.right, rq.dirs, M, s);
        const float pBelow = areaBelow * invTotalSA;
        const float pAbove = areaAbove * invTotalSA;
        const float eb = (c.nAbove == 0 || c.nBelow == 0) ? emptyBonus : 0;
        if (rq.costsFixed) rq.costsFixed[k] = 0;
        if (!rq.kdAware) {
            rq.costs[k] = (float)traversalCost + (float)isectCost * (1 - eb) * (pBelow * (float)c.nBelow + pAbove * (float)c.nAbove);
        } else if (c.d < 3) {
            rq.costs[k] = (float)kdTraversalCost + (float)isectCost * (1 - eb) * (pBelow * (float)c.nBelow + pAbove * (float)c.nAbove);
        } else {
            const float costIntersection = (float)isectCost * (1 - eb) * (pBelow * (float)c.nBelow + pAbove * (float)c.nAbove);
            if (rq.costsFixed) rq.costsFixed[k] = (float)traversalCost + costIntersection;
            rq.costs[k] = BSP_ALPHA * (float)isectCost * (float)(rq.sc.nPrimitives - 1) + (float)kdTraversalCost + costIntersection;
        }
        rq.overflow[k] = 0;
    }
}

void RbspInteriorCounts(const RbspTree &t, uint32_t *kd, uint32_t *bsp) {
    const uint32_t mask = RbspBitMask(t.M);
    uint32_t k = 0, b = 0;
    for (const RbspNode &nd : t.nodes) {
        const uint32_t ax = nd.b & mask;
        if (ax == t.M) continue;
        if (ax < 3) ++k; else ++b;
    }
    *kd = k; *bsp = b;
}

const char *CheckRbspTree(const RbspTree &t, uint32_t *depthOut) {
    const uint32_t M = t.M;
    if (M != 3 && M != 7 && M != 9 && M != 13) return "the tree's direction count is not 3, 7, 9 or 13";
    if (t.directions.size() != 3 * (size_t)M) return "the direction table does not hold M directions";
    return CheckBspNodes(t.nodes, t.primIndices, t.nPrims, M, RbspBitOffset(M), RbspBitMask(M), depthOut);
}

}  // namespace hprt
