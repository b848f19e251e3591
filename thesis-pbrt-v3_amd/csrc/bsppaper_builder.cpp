// hprt — BSPPaper::buildTree (accelerators/bspPaper.cpp:34-305) with KDOPMeshWithDirections (kDOPMesh.h:238-266),
// Triangle::getBSPPaperPlanes (shapes/triangle.cpp:678-720) and BVHAccel's two plane classifications (accelerators/bvh.cpp:439-527),
// restated operation for operation.  Every float operation is one IEEE rounding in the reference's order (built with
// -ffp-contract=off); Cross is computed in double, as pbrt's Cross does.
//
// The one liberty, as in the RBSP builder: the candidates of a node may be costed on several threads.  Each candidate's cost is a
// pure function of the node's k-DOP, its BVH and the candidate, and the reduction keeps the first minimum in the reference's scan
// order (axis candidates by axis and edge, then plane candidates by primitive and plane), so the tree does not depend on the
// thread count.  The winner's two halves are then cut and measured once more, exactly as the scan left them.  For the same reason
// a node's candidates may be costed elsewhere altogether (BspPaperParams::costFn: the device-assisted build, bsp_cost.h), as long
// as every cost, fixed cost and count carries the bits CostOne below would give; what the hook flags is costed here again.
//
// BspPaperParams::kdAware selects BSPPaperKd::buildTree (accelerators/bspPaperKd.cpp:34-339) over BSPKdNode (BSPKd.h:11-174): the
// same scan with the kd-aware costs, a second minimum over the plane candidates alone, and the 3-bit node flags.
#include "bsppaper_builder.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <limits>
#include <thread>
#include "bsp_build.h"
#include "bvh_builder.h"

namespace hprt {
namespace {

using namespace bspbuild;     // the vector helpers, PrimBounds, the sweep's types, CutMeasure

// The BVH a node builds over its primitives (BVHAccel(currentPrimitives, 4, 8, 1)); local primitive i is global primNums[i]
struct NodeBvh {
    const float *bmin, *bmax, *tri9; const uint8_t *isTri;
    const uint32_t *primNums;
    BvhTree bvh;
    std::vector<float> lo, hi;

    void build(size_t n) {
        lo.resize(3 * n); hi.resize(3 * n);
        for (size_t i = 0; i < n; ++i)
            for (int k = 0; k < 3; ++k) { lo[3 * i + k] = bmin[3 * (size_t)primNums[i] + k]; hi[3 * i + k] = bmax[3 * (size_t)primNums[i] + k]; }
        BuildBvh(n, lo.data(), hi.data(), 1, 4, 8, &bvh);
    }
    // the node's conservative test: Dot(axis, centre) -+ half the diagonal's length; 0 wholly below, 1 wholly above, 2 straddles
    int side(const BvhNode &nd, const BspPlane &p) const {
        const float dx = nd.bmax[0] - nd.bmin[0], dy = nd.bmax[1] - nd.bmin[1], dz = nd.bmax[2] - nd.bmin[2];   // Diagonal()
        const float maxDiff = std::sqrt(dx * dx + dy * dy + dz * dz) / 2;
        const float half = (float)1 / 2;                                                                        // Vector3::operator/
        const float c[3] = {nd.bmin[0] + dx * half, nd.bmin[1] + dy * half, nd.bmin[2] + dz * half};
        const float centerProjection = p.axis[0] * c[0] + p.axis[1] * c[1] + p.axis[2] * c[2];
        if (centerProjection + maxDiff < p.t) return 0;
        if (centerProjection - maxDiff > p.t) return 1;
        return 2;
    }
    Range leafBounds(uint32_t ordered, const BspPlane &p) const {
        return PrimBounds(bmin, bmax, tri9, isTri, primNums[bvh.primOrder[ordered]], p.axis);
    }
    // getAmountToLeftAndRight (bvh.cpp:439-470): a node wholly on one side adds its primitive count (nPrimitives() of an interior
    // node is its subtree's); a straddling leaf counts each primitive by getBounds, a touching one on both sides
    void count(const BspPlane &p, uint32_t *left, uint32_t *right, std::vector<uint32_t> &stack) const {
        uint32_t l = 0, r = 0;
        stack.clear();
        stack.push_back(0);
        while (!stack.empty()) {
            const uint32_t idx = stack.back();
            stack.pop_back();
            const BvhNode &nd = bvh.nodes[idx];
            const int s = side(nd, p);
            const uint32_t np = nd.countAxis >> 2;
            if (s == 0) l += np;
            else if (s == 1) r += np;
            else if ((nd.countAxis & 3u) == 3u) {
                for (uint32_t i = 0; i < np; ++i) {
                    const Range b = leafBounds((uint32_t)nd.offset + i, p);
                    if (b.min <= p.t) l += 1;
                    if (b.max >= p.t) r += 1;
                }
            } else {
                stack.push_back(idx + 1);
                stack.push_back((uint32_t)nd.offset);
            }
        }
        *left = l; *right = r;
    }
    // getPrimnumsToLeftAndRight (bvh.cpp:472-527): local primitive numbers (primNumMapping), in the order the stack visits the
    // leaves (the second child is pushed last, so it is popped first)
    void split(const BspPlane &p, std::vector<uint32_t> *left, std::vector<uint32_t> *right) const {
        struct E { uint32_t node; uint8_t state; };         // 0 unknown, 1 goes left, 2 goes right
        std::vector<E> stack;
        stack.push_back(E{0, 0});
        auto all = [&](const BvhNode &nd, std::vector<uint32_t> *out) {
            for (uint32_t i = 0; i < (nd.countAxis >> 2); ++i) out->push_back(bvh.primOrder[(uint32_t)nd.offset + i]);
        };
        while (!stack.empty()) {
            const E e = stack.back();
            stack.pop_back();
            const BvhNode &nd = bvh.nodes[e.node];
            const bool leaf = (nd.countAxis & 3u) == 3u;
            const uint8_t state = e.state ? e.state : (uint8_t)(side(nd, p) + 1);      // 1 left, 2 right, 3 straddles
            if (leaf) {
                if (state == 1) all(nd, left);
                else if (state == 2) all(nd, right);
                else
                    for (uint32_t i = 0; i < (nd.countAxis >> 2); ++i) {
                        const Range b = leafBounds((uint32_t)nd.offset + i, p);
                        if (b.min <= p.t) left->push_back(bvh.primOrder[(uint32_t)nd.offset + i]);
                        if (b.max >= p.t) right->push_back(bvh.primOrder[(uint32_t)nd.offset + i]);
                    }
            } else {
                const uint8_t childState = state == 3 ? 0 : state;
                stack.push_back(E{e.node + 1, childState});
                stack.push_back(E{(uint32_t)nd.offset, childState});
            }
        }
    }
};

// k < 3: axis k's edge i (nBelow / nAbove from the sweep); k == 33: plane `plane` of the node's primitives
struct Cand { uint32_t k, i, nBelow, nAbove; BspPlane plane; };
static_assert(sizeof(Cand) == sizeof(bspcost::Cand) && sizeof(Cand) == 32, "bsp_cost.h restates Cand");
static_assert(sizeof(KEdge) == sizeof(kdopcost::Edge) && sizeof(KEdge) == 32, "kdop_cost.h restates KEdge");

// What one candidate's cost reads besides the node, its BVH and the candidate
struct CostConsts {
    bool kdAware; float invTotalSA, emptyBonus; uint32_t isectCost, traversalCost, kdTraversalCost;
};
// One candidate of the scan: costs[k] (and, kd-aware, costsFixed[k]) as the reference's loop body leaves them; a plane
// candidate outside the k-DOP's extent costs +inf and keeps its counts
void CostOne(const BuildNode &cur, const NodeBvh &nb, const CostConsts &cc, Cand &c, Scratch &s, std::vector<float> *candDirs,
             std::vector<uint32_t> &bvhStack, float *cost, float *costFixed) {
    const float BSP_ALPHA = 0.1f;                                    // bspPaperKd.cpp:35
    if (c.k == 33u) {
        Range db{std::numeric_limits<float>::max(), std::numeric_limits<float>::lowest()};
        for (const KEdge &ke : cur.mesh) {
            const float t1 = Dot(c.plane.axis, ke.v1), t2 = Dot(c.plane.axis, ke.v2);
            db = Range{fmin_std(db.min, fmin_std(t1, t2)), fmax_std(db.max, fmax_std(t1, t2))};
        }
        if (!(c.plane.t > db.min && c.plane.t < db.max)) { *cost = std::numeric_limits<float>::infinity(); return; }
    }
    float areaBelow, areaAbove;
    CutMeasure(cur, c.plane.t, c.plane.axis, s, candDirs, &areaBelow, &areaAbove);
    const float pBelow = areaBelow * cc.invTotalSA;
    const float pAbove = areaAbove * cc.invTotalSA;
    if (c.k == 33u) nb.count(c.plane, &c.nBelow, &c.nAbove, bvhStack);
    const float eb = (c.nAbove == 0 || c.nBelow == 0) ? cc.emptyBonus : 0;
    if (!cc.kdAware) *cost = (float)cc.traversalCost + (float)cc.isectCost * (1 - eb) * (pBelow * (float)c.nBelow + pAbove * (float)c.nAbove);
    else if (c.k != 33u) *cost = (float)cc.kdTraversalCost + (float)cc.isectCost * (1 - eb) * (pBelow * (float)c.nBelow + pAbove * (float)c.nAbove);
    else {                                               // bspPaperKd.cpp:215-218
        const float costIntersection = (float)cc.isectCost * (1 - eb) * (pBelow * (float)c.nBelow + pAbove * (float)c.nAbove);
        *costFixed = (float)cc.traversalCost + costIntersection;
        *cost = BSP_ALPHA * (float)cc.isectCost * (float)(cur.nPrimitives - 1) + (float)cc.kdTraversalCost + costIntersection;
    }
}

}  // namespace

void BspBvhRecords(const BvhNode *nodes, size_t n, bspcost::BvhRec *out) {
    for (size_t k = 0; k < n; ++k) {
        const BvhNode &nd = nodes[k];
        // (NodeBvh::side, operation for operation)
        const float dx = nd.bmax[0] - nd.bmin[0], dy = nd.bmax[1] - nd.bmin[1], dz = nd.bmax[2] - nd.bmin[2];
        const float maxDiff = std::sqrt(dx * dx + dy * dy + dz * dz) / 2;
        const float half = (float)1 / 2;
        out[k] = bspcost::BvhRec{{nd.bmin[0] + dx * half, nd.bmin[1] + dy * half, nd.bmin[2] + dz * half}, maxDiff, nd.offset, nd.countAxis, 0u, 0u};
    }
}

void BspCostVector(const BspCostRequest &rq) {
    BuildNode cur{0u, rq.sc.nPrimitives, 0u, Mesh(), std::vector<float>(rq.dirs, rq.dirs + 3 * (size_t)rq.M), 0.f, 0, 0u};
    cur.mesh.resize(rq.nEdges);
    if (rq.nEdges) std::memcpy(static_cast<void *>(cur.mesh.data()), rq.mesh, (size_t)rq.nEdges * sizeof(KEdge));
    NodeBvh nb{rq.bmin, rq.bmax, rq.tri9, rq.isTri, rq.primNums, {}, {}, {}};
    nb.bvh.nodes.assign(rq.bvhNodes, rq.bvhNodes + rq.nBvh);
    nb.bvh.primOrder.assign(rq.primOrder, rq.primOrder + (rq.nBvh ? rq.nPrims : 0u));
    const CostConsts cc{rq.kdAware, rq.sc.invTotalSA, rq.sc.emptyBonus, rq.sc.isectCost, rq.sc.traversalCost, rq.sc.kdTraversalCost};
    Scratch s;
    std::vector<float> candDirs;
    std::vector<uint32_t> bvhStack;
    Cand *cands = reinterpret_cast<Cand *>(rq.cands);
    for (size_t k = 0; k < rq.n; ++k) {
        float fixed = std::numeric_limits<float>::infinity();
        CostOne(cur, nb, cc, cands[k], s, &candDirs, bvhStack, &rq.costs[k], &fixed);
        if (rq.costsFixed) rq.costsFixed[k] = fixed;
        rq.overflow[k] = 0;
    }
}

std::vector<BspPlane> BspPaperTrianglePlanes(const float *p9) {
    std::vector<BspPlane> planes;
    const float *p0 = p9, *p1 = p9 + 3, *p2 = p9 + 6;
    // Triangle::Normal (shapes/triangle.cpp:584-594)
    V n = Cross(Sub(p0, p2), Sub(p1, p2));
    if (Length(n) > 0) n = Normalize(n);
    auto add = [&](const V &a, const float *p) { planes.push_back(BspPlane{DotP(a, p), {a.x, a.y, a.z}}); };
    if (Length(n) > 0) {
        n = PositiveX(n);
        add(n, p0);
        V axis = Cross(n, Sub(p0, p1));
        if (Length(axis) > 0) add(PositiveX(axis), p0);
        axis = Cross(n, Sub(p0, p2));
        if (Length(axis) > 0) add(PositiveX(axis), p0);
        axis = Cross(n, Sub(p1, p2));
        if (Length(axis) > 0) add(PositiveX(axis), p1);
    }
    return planes;
}

void BspPaperClassify(size_t n, const float *bmin, const float *bmax, const float *tri9, const uint8_t *isTri, const BspPlane &plane,
                      uint32_t counts[2], std::vector<uint32_t> *left, std::vector<uint32_t> *right) {
    std::vector<uint32_t> ident(n);
    for (size_t i = 0; i < n; ++i) ident[i] = (uint32_t)i;
    NodeBvh nb{bmin, bmax, tri9, isTri, ident.data(), {}, {}, {}};
    nb.build(n);
    std::vector<uint32_t> stack;
    nb.count(plane, &counts[0], &counts[1], stack);
    nb.split(plane, left, right);
}

std::string BuildBspPaperTree(size_t n, const float *bmin, const float *bmax, const float *tri9, const uint8_t *isTri, const BspPaperParams &p,
                              BspPaperTree *out) {
    BspPaperTree &t = *out;
    t = BspPaperTree();
    // CreateBSPPaperTreeAccelerator / GenericBSP: the parameters as the reference holds them (uint32_t, Float)
    const uint32_t isectCost = (uint32_t)p.isectCost, traversalCost = (uint32_t)p.travCost, maxPrims = (uint32_t)p.maxPrims;
    const bool kdAware = p.kdAware;
    const uint32_t kdTraversalCost = (uint32_t)p.kdTravCost;
    t.kdAware = kdAware;
    const uint32_t off = kdAware ? (uint32_t)BSPPAPERKD_OFF : (uint32_t)BSPPAPER_OFF;
    const float emptyBonus = p.emptyBonus;
    uint32_t maxDepth = (uint32_t)p.maxDepth;
    if (maxDepth == (uint32_t)-1) maxDepth = (uint32_t)std::round(2 + 1.6f * (float)Log2Int64((uint64_t)n));   // calculateMaxDepth
    t.nPrims = (uint32_t)n; t.maxDepth = maxDepth;
    const int nThreads = ThreadCount(p.threads);

    float lo[3], hi[3];
    for (int k = 0; k < 3; ++k) { lo[k] = std::numeric_limits<float>::max(); hi[k] = std::numeric_limits<float>::lowest(); }
    for (size_t i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) { lo[k] = fmin_std(lo[k], bmin[3 * i + k]); hi[k] = fmax_std(hi[k], bmax[3 * i + k]); }
    for (int k = 0; k < 3; ++k) { t.bounds[k] = lo[k]; t.bounds[3 + k] = hi[k]; }
    // every primitive's planes (getBSPPaperPlanes: triangles only), in primitive order
    std::vector<uint32_t> planeBegin(n + 1, 0);
    std::vector<BspPlane> allPlanes;
    for (size_t i = 0; i < n; ++i) {
        if (isTri[i]) for (const BspPlane &pl : BspPaperTrianglePlanes(tri9 + 9 * i)) allPlanes.push_back(pl);
        planeBegin[i + 1] = (uint32_t)allPlanes.size();
    }

    // Bounds3::toKDOPMesh (core/geometry.h:1001-1027): the 12 edges of the box with their face ids, and the three axis directions
    Mesh rootMesh;
    {
        const P3 v1{lo[0], lo[1], lo[2]}, v2{lo[0], lo[1], hi[2]}, v3{lo[0], hi[1], lo[2]}, v4{hi[0], lo[1], lo[2]};
        const P3 v5{lo[0], hi[1], hi[2]}, v6{hi[0], lo[1], hi[2]}, v7{hi[0], hi[1], lo[2]}, v8{hi[0], hi[1], hi[2]};
        rootMesh = {{v1, v2, 1, 3}, {v1, v3, 1, 5}, {v1, v4, 3, 5}, {v2, v5, 1, 4}, {v2, v6, 3, 4}, {v3, v5, 1, 2},
                    {v3, v7, 2, 5}, {v4, v6, 0, 3}, {v4, v7, 0, 5}, {v5, v8, 2, 4}, {v6, v8, 0, 4}, {v7, v8, 0, 2}};
    }
    static const float kAxes[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    std::vector<float> rootDirs(kAxes, kAxes + 9);
    std::vector<Scratch> scratch((size_t)nThreads);
    const float rootArea = SurfaceArea(rootMesh, rootDirs.data(), 3, scratch[0]);    // evaluated before the mesh is stored

    std::vector<std::vector<BoundEdge>> edges(3);
    for (auto &e : edges) e.resize(2 * n);
    // the reference's primitive buffer: (maxDepth + 1) * N entries, written without a check; here a write past it is an error
    const uint64_t primsCap = ((uint64_t)maxDepth + 1) * (uint64_t)n;
    std::vector<uint32_t> prims(n + 1);
    for (size_t i = 0; i < n; ++i) prims[i] = (uint32_t)i;

    std::vector<BspNode> &nodes = t.nodes;
    auto initLeaf = [&](const uint32_t *primNums, uint32_t np) {     // treeInitLeaf (BSP.h:11-24)
        BspNode nd;
        nd.b = kdAware ? (BSPPAPERKD_LEAF | (np << BSPPAPERKD_OFF)) : (1u | (np << 1));     // BSPKdNode::initLeaf (BSPKd.h:21-34)
        if (np == 0) nd.a = 0u;
        else if (np == 1) nd.a = primNums[0];
        else {
            nd.a = (uint32_t)t.primIndices.size();
            for (uint32_t i = 0; i < np; ++i) t.primIndices.push_back(primNums[i]);
        }
        nodes.push_back(nd);
        t.axes.insert(t.axes.end(), 3, 0.f);
        ++t.leaves;
    };

    std::vector<Cand> cands;
    std::vector<float> costs, costsFixed;                            // costsFixed: kdAware only, traversalCost + C_isect of a plane candidate
    std::vector<uint8_t> overflow;                                   // per candidate: the costing hook could not cost it (BspPaperParams::costFn)
    std::vector<bspcost::BvhRec> bvhRecs;                            // the node's BVH as the hook reads it
    std::vector<std::vector<uint32_t>> bvhStacks((size_t)nThreads);
    std::vector<std::vector<float>> candDirs((size_t)nThreads);
    std::vector<std::thread> pool;
    uint32_t nodeNum = 0;
    std::vector<BuildNode> stack;
    stack.push_back(BuildNode{maxDepth, (uint32_t)n, 0u, rootMesh, rootDirs, rootArea, 0, (uint32_t)-1});
    while (!stack.empty()) {
        BuildNode cur = std::move(stack.back());
        stack.pop_back();
        if (cur.parentNum != (uint32_t)-1) nodes[cur.parentNum].b |= (nodeNum << off);    // treeSetAboveChild

        if (cur.nPrimitives <= maxPrims || cur.depth == 0) { initLeaf(&prims[cur.primNums], cur.nPrimitives); ++nodeNum; continue; }

        const float oldCost = (float)isectCost * float(cur.nPrimitives);
        const float invTotalSA = 1 / cur.meshArea;
        const uint32_t *primNums = &prims[cur.primNums];
        // the axis sweep's candidates, in the reference's scan order: inside the k-DOP's extent along the axis
        cands.clear();
        for (uint32_t k = 0; k < 3; ++k) {
            Range db{std::numeric_limits<float>::max(), std::numeric_limits<float>::lowest()};
            for (const KEdge &ke : cur.mesh) {
                const float t1 = Dot(kAxes + 3 * k, ke.v1), t2 = Dot(kAxes + 3 * k, ke.v2);
                db = Range{fmin_std(db.min, fmin_std(t1, t2)), fmax_std(db.max, fmax_std(t1, t2))};
            }
            BoundEdge *e = edges[k].data();
            for (uint32_t i = 0; i < cur.nPrimitives; ++i) {
                const uint32_t pn = primNums[i];
                e[2 * i] = BoundEdge{bmin[3 * (size_t)pn + k], pn, EdgeType::Start};
                e[2 * i + 1] = BoundEdge{bmax[3 * (size_t)pn + k], pn, EdgeType::End};
            }
            std::sort(e, e + 2 * cur.nPrimitives, [](const BoundEdge &e0, const BoundEdge &e1) -> bool {
                if (e0.t == e1.t) return (int)e0.type < (int)e1.type;
                else return e0.t < e1.t;
            });
            uint32_t nBelow = 0, nAbove = cur.nPrimitives;
            for (uint32_t i = 0; i < 2 * cur.nPrimitives; ++i) {
                if (e[i].type == EdgeType::End) --nAbove;
                const float edgeT = e[i].t;
                if (edgeT > db.min && edgeT < db.max)
                    cands.push_back(Cand{k, i, nBelow, nAbove, BspPlane{edgeT, {kAxes[3 * k], kAxes[3 * k + 1], kAxes[3 * k + 2]}}});
                if (e[i].type == EdgeType::Start) ++nBelow;
            }
        }
        // then every plane of every primitive, in primNums order (the extent test runs with the costing)
        for (uint32_t i = 0; i < cur.nPrimitives; ++i) {
            const uint32_t pn = primNums[i];
            for (uint32_t q = planeBegin[pn]; q < planeBegin[pn + 1]; ++q) cands.push_back(Cand{33u, q, 0u, 0u, allPlanes[q]});
        }
        NodeBvh nb{bmin, bmax, tri9, isTri, primNums, {}, {}, {}};
        if (planeBegin.back() != 0) nb.build(cur.nPrimitives);
        costs.resize(cands.size());
        if (kdAware) costsFixed.assign(cands.size(), std::numeric_limits<float>::infinity());
        const CostConsts cc{kdAware, invTotalSA, emptyBonus, isectCost, traversalCost, kdTraversalCost};
        auto costRange = [&](size_t k0, size_t k1, int w) {
            for (size_t k = k0; k < k1; ++k)
                CostOne(cur, nb, cc, cands[k], scratch[(size_t)w], &candDirs[(size_t)w], bvhStacks[(size_t)w], &costs[k], kdAware ? &costsFixed[k] : nullptr);
        };
        // the costing hook (BspPaperParams::costFn): the node's candidates costed elsewhere, the flagged ones repaired here
        std::string hookErr;
        const HookResult hooked = RunCostHook(p, cands.size(), overflow, true, [&](BspCostRequest &rq) {
            const bool hasBvh = planeBegin.back() != 0;
            bvhRecs.resize(hasBvh ? nb.bvh.nodes.size() : 0);
            BspBvhRecords(nb.bvh.nodes.data(), bvhRecs.size(), bvhRecs.data());
            size_t nAxis = 0;
            while (nAxis < cands.size() && cands[nAxis].k != 33u) ++nAxis;
            rq.mesh = reinterpret_cast<const kdopcost::Edge *>(cur.mesh.data()); rq.nEdges = (uint32_t)cur.mesh.size();
            rq.dirs = cur.dirs.data(); rq.M = (uint32_t)(cur.dirs.size() / 3); rq.kdAware = kdAware;
            rq.sc = bspcost::Scalars{invTotalSA, emptyBonus, isectCost, traversalCost, kdTraversalCost, cur.nPrimitives, 0u, 0u, 0u, 0u};
            rq.cands = reinterpret_cast<bspcost::Cand *>(cands.data()); rq.n = cands.size(); rq.nAxis = nAxis;
            rq.bvhNodes = nb.bvh.nodes.data(); rq.bvh = bvhRecs.data(); rq.nBvh = (uint32_t)bvhRecs.size();
            rq.primOrder = nb.bvh.primOrder.data(); rq.primNums = primNums; rq.nPrims = cur.nPrimitives;
            rq.bmin = bmin; rq.bmax = bmax; rq.tri9 = tri9; rq.isTri = isTri; rq.nTotal = n;
            rq.costs = costs.data(); rq.costsFixed = kdAware ? costsFixed.data() : nullptr; rq.overflow = overflow.data();
            rq.level = maxDepth - cur.depth;
        }, [&](size_t k) {
            if (kdAware) costsFixed[k] = std::numeric_limits<float>::infinity();
            costRange(k, k + 1, 0);
        }, &hookErr);
        if (hooked == HookResult::Failed) return hookErr;
        if (hooked == HookResult::Costed) {
            // (costs[], costsFixed[] and the plane candidates' counts are complete)
        } else if (nThreads > 1 && cands.size() >= kParallelCandidates) {
            const size_t chunk = (cands.size() + nThreads - 1) / nThreads;
            pool.clear();
            for (int w = 1; w < nThreads; ++w) {
                const size_t k0 = std::min(cands.size(), w * chunk), k1 = std::min(cands.size(), (w + 1) * chunk);
                pool.emplace_back(costRange, k0, k1, w);
            }
            costRange(0, std::min(cands.size(), chunk), 0);
            for (auto &th : pool) th.join();
        } else costRange(0, cands.size(), 0);
        // the reference's scan: strict `<`, so the first minimum in scan order (an out-of-extent plane costs +inf and never wins)
        size_t best = (size_t)-1;
        float bestCost = std::numeric_limits<float>::infinity();
        for (size_t k = 0; k < cands.size(); ++k)
            if (costs[k] < bestCost) { bestCost = costs[k]; best = k; }
        // kdAware: the second minimum (bestCostFixed / bestKFixed), over the plane candidates only; else it stays unset
        size_t bestFixed = (size_t)-1;
        float bestCostFixed = std::numeric_limits<float>::infinity();
        if (kdAware)
            for (size_t k = 0; k < cands.size(); ++k)
                if (cands[k].k == 33u && costsFixed[k] < bestCostFixed) { bestCostFixed = costsFixed[k]; bestFixed = k; }

        // Create leaf if no good splits were found
        if (bestCost > oldCost && bestCostFixed > oldCost) ++cur.badRefines;
        if ((bestCost > 4 * oldCost && bestCostFixed > 4 * oldCost && cur.nPrimitives < 16) || (best == (size_t)-1 && bestFixed == (size_t)-1) ||
            cur.badRefines == 3) {
            initLeaf(&prims[cur.primNums], cur.nPrimitives); ++nodeNum; continue;
        }

        // the winner's halves, measured (and so reoriented) as the scan left them; the fixed minimum's split only where the first
        // minimum is unset (bspPaperKd.cpp:275-278, :318-329: reachable only when no candidate's first cost is finite)
        const Cand win = cands[best != (size_t)-1 ? best : bestFixed];
        Scratch &s = scratch[0];
        std::vector<float> childDirs;
        float areaBelow, areaAbove;
        CutMeasure(cur, win.plane.t, win.plane.axis, s, &childDirs, &areaBelow, &areaAbove);
        Mesh below = s.left, above = s.right;

        // Classify primitives with respect to split: prims1 first, in place, so that child 0's share does not overwrite it
        uint32_t n0 = 0, n1 = 0;
        const size_t prims1 = cur.primNums;
        size_t prims0;
        if (win.k != 33u) {
            ++t.axisNodes;
            const BoundEdge *e = edges[win.k].data();
            for (uint32_t i = win.i + 1; i < 2 * cur.nPrimitives; ++i)
                if (e[i].type == EdgeType::End) prims[prims1 + n1++] = e[i].primNum;
            prims0 = prims1 + n1;
            uint32_t nStart = 0;
            for (uint32_t i = 0; i < win.i; ++i) nStart += e[i].type == EdgeType::Start;
            if ((uint64_t)prims0 + nStart > primsCap)
                return "the build needs more than the reference's (maxDepth + 1) * N primitive slots; lower \"maxdepth\"";
            if (prims.size() < prims0 + nStart + 1) prims.resize(prims0 + nStart + 1);
            for (uint32_t i = 0; i < win.i; ++i)
                if (e[i].type == EdgeType::Start) prims[prims0 + n0++] = e[i].primNum;
        } else {
            ++t.planeNodes;
            std::vector<uint32_t> left, right;
            nb.split(win.plane, &left, &right);
            for (uint32_t &x : left) x = prims[cur.primNums + x];       // local -> the node's primitive numbers
            for (uint32_t &x : right) x = prims[cur.primNums + x];
            if ((uint64_t)prims1 + right.size() + left.size() > primsCap)
                return "the build needs more than the reference's (maxDepth + 1) * N primitive slots; lower \"maxdepth\"";
            if (prims.size() < prims1 + right.size() + left.size() + 1) prims.resize(prims1 + right.size() + left.size() + 1);
            for (uint32_t x : right) prims[prims1 + n1++] = x;
            prims0 = prims1 + n1;
            for (uint32_t x : left) prims[prims0 + n0++] = x;
        }

        BspNode nd;                                    // treeInitInterior (BSP.h:32-37)
        std::memcpy(&nd.a, &win.plane.t, 4);
        nd.b = !kdAware ? 0u : (win.k != 33u ? win.k : BSPPAPERKD_PLANE);     // BSPKdNode::initInteriorKd / initInterior (BSPKd.h:40-49)
        nodes.push_back(nd);
        if (kdAware && win.k != 33u) t.axes.insert(t.axes.end(), 3, 0.f);     // a kd node holds no axis (the reference leaves it unset)
        else t.axes.insert(t.axes.end(), win.plane.axis, win.plane.axis + 3);
        stack.push_back(BuildNode{cur.depth - 1, n1, cur.badRefines, std::move(above), childDirs, areaAbove, prims1, nodeNum});
        stack.push_back(BuildNode{cur.depth - 1, n0, cur.badRefines, std::move(below), std::move(childDirs), areaBelow, prims0, (uint32_t)-1});
        ++nodeNum;
    }
    uint32_t depth = 0;
    (void)(kdAware ? CheckBspPaperKdTree(t, &depth) : CheckBspPaperTree(t, &depth));
    t.depth = depth;
    return "";
}

const char *CheckBspPaperTree(const BspPaperTree &t, uint32_t *depthOut) {
    if (t.axes.size() != 3 * t.nodes.size()) return "the axis array does not hold one axis per node";
    for (size_t k = 0; k < t.nodes.size(); ++k) {
        if (t.nodes[k].b & BSPPAPER_MASK) continue;
        const float *a = &t.axes[3 * k];
        if (!std::isfinite(a[0]) || !std::isfinite(a[1]) || !std::isfinite(a[2])) return "an interior node's axis is not finite";
        if (a[0] == 0 && a[1] == 0 && a[2] == 0) return "an interior node's axis is zero";
    }
    return CheckBspNodes(t.nodes, t.primIndices, t.nPrims, BSPPAPER_M, BSPPAPER_OFF, BSPPAPER_MASK, depthOut);
}

}  // namespace hprt

namespace hprt {
const char *CheckBspPaperKdTree(const BspPaperTree &t, uint32_t *depthOut) {
    if (t.axes.size() != 3 * t.nodes.size()) return "the axis array does not hold one axis per node";
    // CheckBspNodes over M = 3 takes directions 0-2 and the leaf tag 3: a plane node stands in as direction 0 once its axis is checked
    std::vector<BspNode> nodes(t.nodes);
    for (size_t k = 0; k < nodes.size(); ++k) {
        const uint32_t kind = nodes[k].b & BSPPAPERKD_MASK;
        if (kind > BSPPAPERKD_PLANE) return "a node's flags name no node kind";
        if (kind != BSPPAPERKD_PLANE) continue;
        const float *a = &t.axes[3 * k];
        if (!std::isfinite(a[0]) || !std::isfinite(a[1]) || !std::isfinite(a[2])) return "an interior node's axis is not finite";
        if (a[0] == 0 && a[1] == 0 && a[2] == 0) return "an interior node's axis is zero";
        nodes[k].b &= ~BSPPAPERKD_MASK;
    }
    return CheckBspNodes(nodes, t.primIndices, t.nPrims, BSPPAPERKD_LEAF, BSPPAPERKD_OFF, BSPPAPERKD_MASK, depthOut);
}
}  // namespace hprt
