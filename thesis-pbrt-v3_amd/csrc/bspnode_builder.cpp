// hprt — BSPNodeBased::buildTree (accelerators/bspNodeBased.cpp:27-223), BSPNodeBasedWithKd::buildTree (bspNodeBasedWithKd.cpp) and
// BSPNodeBasedFastKd::buildTree (bspNodeBasedFastKd.cpp:28-330) with the direction choosers chooseArbitraryNormals /
// chooseRandomDirections (randomNormals.h) and calculateClusterMeans (clustering.h), restated operation for operation.  Every
// float operation is one IEEE rounding in the reference's order (built with -ffp-contract=off); the engine is std::mt19937 and the
// distributions std::uniform_real_distribution<>, drawn from exactly as the reference draws, on the calling thread and in node order.
//
// Two liberties.  The seed is a parameter (bspnode_builder.h).  And, as in the other builders, the candidates of a node may be costed
// on several threads: each candidate's cost is a pure function of the node's k-DOP, the direction and the candidate, and the
// reduction keeps the first minimum in the reference's scan order (direction, then edge) — for the fastkd form each of its two
// minima — so the tree does not depend on the thread count.  The winner's two halves are then cut and measured once more, exactly
// as the scan left them.  For the same reason a node's candidates may be costed elsewhere altogether (BspNodeParams::costFn: the
// device-assisted build, bspnode_cost.h), as long as every cost and fixed cost carries the bits CostOne below would give; what the
// hook flags is costed here again.
#include "bspnode_builder.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <limits>
#include <random>
#include <set>
#include <thread>
#include "bsp_build.h"

namespace hprt {
namespace {

using namespace bspbuild;

struct Cand { uint32_t k, i, nBelow, nAbove; float t; };     // direction k's edge i
static_assert(sizeof(KEdge) == sizeof(kdopcost::Edge) && sizeof(KEdge) == 32, "kdop_cost.h restates KEdge");

// What one candidate's cost reads besides the node, the direction and the candidate
struct CostConsts {
    bool fastKd; float invTotalSA, emptyBonus; uint32_t isectCost, traversalCost, kdTraversalCost;
};
// One candidate of the scan: costs[k] (and, for a fastkd chosen direction, costsFixed[k]) as the reference's loop body leaves
// them.  d: the candidate's direction; kdAxis: one of fastkd's three axes.
void CostOne(const BuildNode &cur, const CostConsts &cc, const float *d, bool kdAxis, uint32_t nBelow, uint32_t nAbove, float t, Scratch &s,
             std::vector<float> *candDirs, float *cost, float *costFixed) {
    const float BSP_ALPHA = 0.1;                                     // bspNodeBasedFastKd.cpp:29
    float areaBelow, areaAbove;
    CutMeasure(cur, t, d, s, candDirs, &areaBelow, &areaAbove);
    const float pBelow = areaBelow * cc.invTotalSA;
    const float pAbove = areaAbove * cc.invTotalSA;
    const float eb = (nAbove == 0 || nBelow == 0) ? cc.emptyBonus : 0;
    if (!cc.fastKd) *cost = (float)cc.traversalCost + (float)cc.isectCost * (1 - eb) * (pBelow * (float)nBelow + pAbove * (float)nAbove);
    else if (kdAxis) *cost = (float)cc.kdTraversalCost + (float)cc.isectCost * (1 - eb) * (pBelow * (float)nBelow + pAbove * (float)nAbove);
    else {                                               // bspNodeBasedFastKd.cpp:237-239
        const float costIntersection = (float)cc.isectCost * (1 - eb) * (pBelow * (float)nBelow + pAbove * (float)nAbove);
        *costFixed = (float)cc.traversalCost + costIntersection;
        *cost = BSP_ALPHA * (float)cc.isectCost * (float)(cur.nPrimitives - 1) + (float)cc.kdTraversalCost + costIntersection;
    }
}

// Primitive::Normal: Triangle::Normal (shapes/triangle.cpp:584-594); every other shape's is (0, 0, 0) (core/shape.h:94-96)
V PrimNormal(const float *tri9, const uint8_t *isTri, uint32_t pn) {
    if (!isTri[pn]) return V{0, 0, 0};
    const float *p0 = tri9 + 9 * (size_t)pn, *p1 = p0 + 3, *p2 = p0 + 6;
    V n = Cross(Sub(p0, p2), Sub(p1, p2));
    if (Length(n) > 0) n = Normalize(n);
    return n;
}
inline float DotV(const V &a, const V &b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
// Angle (core/geometry.h:1270-1272)
inline float Angle(const V &a, const V &b) { return std::acos(std::max(std::min((float)1.0, DotV(a, b)), (float)-1.0)); }

const char *const kDrawnNp = "a drawn primitive index equals the node's primitive count: the reference reads past its primitives there";

// random_int (clustering.h:48-51): a double in [from, to) truncated to uint32_t
inline uint32_t RandomInt(std::mt19937 &gen, uint32_t from, uint32_t to) {
    std::uniform_real_distribution<> dis(from, to);
    return uint32_t(dis(gen));
}
// `while (nIds.size() < count) nIds.insert(random_int(gen, 0, np))`; false when an index equal to np is drawn
bool DrawIds(std::mt19937 &gen, uint32_t count, uint32_t np, std::set<uint32_t> *nIds) {
    while (nIds->size() < count) {
        const uint32_t id = RandomInt(gen, 0, np);
        if (id >= np) return false;
        nIds->insert(id);
    }
    return true;
}

struct Chooser {
    int kind;
    const float *tri9; const uint8_t *isTri;
    std::mt19937 gen;

    V normal(uint32_t pn) const { return PositiveX(PrimNormal(tri9, isTri, pn)); }

    // chooseArbitraryNormals (randomNormals.h:13-26)
    const char *arbitrary(uint32_t K, const uint32_t *primNums, uint32_t np, std::vector<V> *out) {
        std::set<uint32_t> nIds;
        if (!DrawIds(gen, std::min(np, K), np, &nIds)) return kDrawnNp;
        for (uint32_t id : nIds) out->push_back(normal(primNums[id]));
        return nullptr;
    }
    // chooseRandomDirections (randomNormals.h:28-46)
    const char *random(uint32_t K, std::vector<V> *out) {
        const float Pi = 3.14159265358979323846;
        std::uniform_real_distribution<> disPhi(0, 2 * Pi);
        std::uniform_real_distribution<> disCosTheta(-1, 1);
        for (uint32_t i = 0; i < K; i++) {
            const float phi = disPhi(gen);
            const float cosTheta = disCosTheta(gen);
            const float theta = std::acos(cosTheta);
            const float x = std::sin(theta) * std::cos(phi);
            const float y = std::sin(theta) * std::sin(phi);
            const float z = std::cos(theta);
            out->push_back(PositiveX(V{x, y, z}));
        }
        return nullptr;
    }
    // calculateClusterMeans (clustering.h:53-112)
    const char *cluster(uint32_t K, const uint32_t *primNums, uint32_t np, std::vector<V> *out) {
        std::vector<V> normals;
        normals.reserve(np);
        for (uint32_t i = 0; i < np; ++i) normals.push_back(normal(primNums[i]));
        if (np <= K) { *out = normals; return nullptr; }

        std::set<uint32_t> nIds;
        if (!DrawIds(gen, K, np, &nIds)) return kDrawnNp;
        std::vector<V> clusterMeans, newClusterMeans;
        std::vector<std::vector<V>> clusters;
        for (uint32_t id : nIds) { clusterMeans.push_back(normals[id]); clusters.emplace_back(); }
        newClusterMeans = clusterMeans;
        auto maxDifference = [](const std::vector<V> &a, const std::vector<V> &b) {      // calculateMaxDifference
            float maxDiff = 0;
            for (size_t i = 0; i < a.size(); ++i) {
                const V diff{a[i].x - b[i].x, a[i].y - b[i].y, a[i].z - b[i].z};
                maxDiff = std::max(maxDiff, DotV(diff, diff));
            }
            return maxDiff;
        };
        auto closestMean = [](const V &n, const std::vector<V> &means) {                  // calculateIdOfClosestMean
            uint32_t closest = 0;
            float closestAngle = Angle(n, means[0]);
            for (uint32_t i = 1; i < means.size(); ++i) {
                const float currentAngle = Angle(n, means[i]);
                if (currentAngle < closestAngle) { closest = i; closestAngle = currentAngle; }
            }
            return closest;
        };
        const uint32_t maxIterations = 500;
        uint32_t iterations = 0;
        while (iterations < maxIterations && (iterations == 0 || maxDifference(clusterMeans, newClusterMeans) > 0.000001)) {
            ++iterations;
            clusterMeans = newClusterMeans;
            for (const V &n : normals) clusters[closestMean(n, clusterMeans)].push_back(n);
            for (uint32_t i = 0; i < K; ++i) {
                if (clusters[i].empty()) {      // an empty cluster: every mean is drawn again
                    std::set<uint32_t> again;
                    if (!DrawIds(gen, K, np, &again)) return kDrawnNp;
                    const std::vector<uint32_t> v(again.begin(), again.end());
                    for (uint32_t ii = 0; ii < K; ++ii) { newClusterMeans[ii] = normals[v[ii]]; clusters[ii].clear(); }
                    break;
                }
                V sum{0, 0, 0};                 // calculateMeanVector
                for (const V &c : clusters[i]) { sum.x += c.x; sum.y += c.y; sum.z += c.z; }
                newClusterMeans[i] = Normalize(sum);
                clusters[i].clear();
            }
        }
        *out = newClusterMeans;
        return nullptr;
    }
    // calculateDirections of the nine classes
    const char *choose(uint32_t K, const uint32_t *primNums, uint32_t np, std::vector<V> *out) {
        out->clear();
        if (kind == BSPNODE_ARBITRARY) return arbitrary(K, primNums, np, out);
        if (kind == BSPNODE_RANDOM) return random(K, out);
        return cluster(K, primNums, np, out);
    }
};

}  // namespace

bool BspNodeAccelerator(const std::string &name, int *chooser, int *form) {
    static const char *const kChoosers[3] = {"bsparbitrary", "bspcluster", "bsprandom"};
    static const char *const kForms[3] = {"", "withkd", "fastkd"};
    for (int c = 0; c < 3; ++c)
        for (int f = 0; f < 3; ++f)
            if (name == std::string(kChoosers[c]) + kForms[f]) { *chooser = c; *form = f; return true; }
    return false;
}

void BspNodeCostVector(const BspNodeCostRequest &rq) {
    BuildNode cur{0u, rq.sc.nPrimitives, 0u, Mesh(), std::vector<float>(rq.dirs, rq.dirs + 3 * (size_t)rq.M), 0.f, 0, 0u};
    cur.mesh.resize(rq.nEdges);
    if (rq.nEdges) std::memcpy(static_cast<void *>(cur.mesh.data()), rq.mesh, (size_t)rq.nEdges * sizeof(KEdge));
    const CostConsts cc{rq.fastKd, rq.sc.invTotalSA, rq.sc.emptyBonus, rq.sc.isectCost, rq.sc.traversalCost, rq.sc.kdTraversalCost};
    Scratch s;
    std::vector<float> candDirs;
    for (size_t k = 0; k < rq.n; ++k) {
        const bspnodecost::Cand &c = rq.cands[k];
        const bspnodecost::SweepDir &sd = rq.sweep[c.k];
        float fixed = std::numeric_limits<float>::infinity();
        CostOne(cur, cc, sd.axis, sd.kind != bspnodecost::KIND_CHOSEN, c.nBelow, c.nAbove, c.t, s, &candDirs, &rq.costs[k], &fixed);
        if (rq.costsFixed) rq.costsFixed[k] = fixed;
        rq.overflow[k] = 0;
    }
}

std::string BspNodeChoose(int chooser, uint32_t K, uint32_t seed, size_t n, const float *tri9, uint32_t draws, std::vector<uint32_t> *counts,
                          std::vector<float> *dirs) {
    const std::vector<uint8_t> isTri(n, 1);
    std::vector<uint32_t> primNums(n);
    for (size_t i = 0; i < n; ++i) primNums[i] = (uint32_t)i;
    Chooser ch{chooser, tri9, isTri.data(), std::mt19937(seed)};
    std::vector<V> out;
    for (uint32_t k = 0; k < draws; ++k) {
        if (const char *err = ch.choose(K, primNums.data(), (uint32_t)n, &out)) return err;
        counts->push_back((uint32_t)out.size());
        for (const V &v : out) { dirs->push_back(v.x); dirs->push_back(v.y); dirs->push_back(v.z); }
    }
    return "";
}

std::string BspNodeRefuseParams(const BspNodeParams &p) {
    if (p.chooser < BSPNODE_ARBITRARY || p.chooser > BSPNODE_RANDOM || p.form < BSPNODE_PLAIN || p.form > BSPNODE_FASTKD)
        return "unknown direction chooser or tree form";
    const bool withKd = p.form == BSPNODE_WITHKD, fastKd = p.form == BSPNODE_FASTKD;
    // K - 3 wraps in the reference for K < 3 and edges[k] is indexed past its end
    if ((withKd || fastKd) && p.nDirections < 3)
        return "nbDirections " + std::to_string(p.nDirections) + " is not supported: the withkd and fastkd trees take the three axes and K - 3 chosen directions";
    // calculateClusterMeans over K = 0 means reads means[0] of an empty list
    if (p.chooser == BSPNODE_CLUSTER && !withKd && !fastKd && p.nDirections < 1)
        return "nbDirections " + std::to_string(p.nDirections) + " is not supported: bspcluster needs at least one direction";
    if (p.nDirections < 0 || p.nDirections > 4096) return "nbDirections " + std::to_string(p.nDirections) + " is not supported";
    return "";
}

std::string BuildBspNodeTree(size_t n, const float *bmin, const float *bmax, const float *tri9, const uint8_t *isTri, const BspNodeParams &p,
                             BspPaperTree *out) {
    BspPaperTree &t = *out;
    t = BspPaperTree();
    const std::string refused = BspNodeRefuseParams(p);
    if (!refused.empty()) return refused;
    const bool withKd = p.form == BSPNODE_WITHKD, fastKd = p.form == BSPNODE_FASTKD;
    const uint32_t K = (uint32_t)p.nDirections;
    const uint32_t nFixed = (withKd || fastKd) ? 3u : 0u, Kchosen = K - nFixed;
    // Create...TreeAccelerator / GenericBSP: the parameters as the reference holds them (uint32_t, Float)
    const uint32_t isectCost = (uint32_t)p.isectCost, traversalCost = (uint32_t)p.travCost, maxPrims = (uint32_t)p.maxPrims;
    const uint32_t kdTraversalCost = (uint32_t)p.kdTravCost;
    const float emptyBonus = p.emptyBonus;
    t.kdAware = fastKd;
    const uint32_t off = fastKd ? (uint32_t)BSPPAPERKD_OFF : (uint32_t)BSPPAPER_OFF;
    uint32_t maxDepth = (uint32_t)p.maxDepth;
    if (maxDepth == (uint32_t)-1) maxDepth = (uint32_t)std::round(2 + 1.6f * (float)Log2Int64((uint64_t)n));   // calculateMaxDepth
    t.nPrims = (uint32_t)n; t.maxDepth = maxDepth;
    const int nThreads = ThreadCount(p.threads);
    Chooser chooser{p.chooser, tri9, isTri, std::mt19937(p.seed)};

    float lo[3], hi[3];
    for (int k = 0; k < 3; ++k) { lo[k] = std::numeric_limits<float>::max(); hi[k] = std::numeric_limits<float>::lowest(); }
    for (size_t i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) { lo[k] = fmin_std(lo[k], bmin[3 * i + k]); hi[k] = fmax_std(hi[k], bmax[3 * i + k]); }
    for (int k = 0; k < 3; ++k) { t.bounds[k] = lo[k]; t.bounds[3 + k] = hi[k]; }

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

    std::vector<std::vector<BoundEdge>> edges(K);
    for (auto &e : edges) e.resize(2 * n);
    // the reference's primitive buffer: (maxDepth + 1) * N entries, written without a check; here a write past it is an error
    const uint64_t primsCap = ((uint64_t)maxDepth + 1) * (uint64_t)n;
    std::vector<uint32_t> prims(n + 1);
    for (size_t i = 0; i < n; ++i) prims[i] = (uint32_t)i;

    std::vector<BspNode> &nodes = t.nodes;
    auto initLeaf = [&](const uint32_t *primNums, uint32_t np) {     // treeInitLeaf (BSP.h:11-24) / BSPKdNode::initLeaf (BSPKd.h:21-34)
        BspNode nd;
        nd.b = fastKd ? (BSPPAPERKD_LEAF | (np << BSPPAPERKD_OFF)) : (1u | (np << 1));
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
    std::vector<float> costs, costsFixed;       // costsFixed: fastkd's traversalCost + C_isect of a chosen direction's candidate
    std::vector<uint8_t> overflow;              // per candidate: the costing hook could not cost it (BspNodeParams::costFn)
    std::vector<bspnodecost::Cand> hookCands;   // the candidates and the sweep's directions as the hook reads them
    std::vector<bspnodecost::SweepDir> hookDirs;
    std::vector<V> chosen;
    std::vector<float> nodeDirs;                // the node's directions, 3 floats each: the fixed axes, then the chosen ones
    std::vector<std::vector<float>> candDirs((size_t)nThreads);
    std::vector<std::thread> pool;
    uint32_t nodeNum = 0;
    std::vector<BuildNode> stack;
    stack.push_back(BuildNode{maxDepth, (uint32_t)n, 0u, rootMesh, rootDirs, rootArea, 0, (uint32_t)-1});
    while (!stack.empty()) {
        BuildNode cur = std::move(stack.back());
        stack.pop_back();
        if (cur.parentNum != (uint32_t)-1) nodes[cur.parentNum].b |= (nodeNum << off);    // treeSetAboveChild / setAboveChild

        if (cur.nPrimitives <= maxPrims || cur.depth == 0) { initLeaf(&prims[cur.primNums], cur.nPrimitives); ++nodeNum; continue; }

        const float oldCost = (float)isectCost * float(cur.nPrimitives);
        const float invTotalSA = 1 / cur.meshArea;
        const uint32_t *primNums = &prims[cur.primNums];
        // the node's directions.  (The fastkd form sweeps its axes before it draws; the sweeps draw nothing, so the order of the
        // draws is the reference's.)
        nodeDirs.assign(kAxes, kAxes + 3 * nFixed);
        if (Kchosen > 0 || nFixed == 0) {
            if (const char *err = chooser.choose(Kchosen, primNums, cur.nPrimitives, &chosen)) return err;
            for (const V &v : chosen) { nodeDirs.push_back(v.x); nodeDirs.push_back(v.y); nodeDirs.push_back(v.z); }
        }
        const uint32_t nDirs = (uint32_t)(nodeDirs.size() / 3);

        // every candidate of every direction, in the reference's scan order: strictly inside the k-DOP's extent along the direction
        cands.clear();
        for (uint32_t k = 0; k < nDirs; ++k) {
            const float *d = &nodeDirs[3 * k];
            Range db{std::numeric_limits<float>::max(), std::numeric_limits<float>::lowest()};
            for (const KEdge &ke : cur.mesh) {
                const float t1 = Dot(d, ke.v1), t2 = Dot(d, ke.v2);
                db = Range{fmin_std(db.min, fmin_std(t1, t2)), fmax_std(db.max, fmax_std(t1, t2))};
            }
            BoundEdge *e = edges[k].data();
            for (uint32_t i = 0; i < cur.nPrimitives; ++i) {
                const uint32_t pn = primNums[i];
                // fastkd's axes take the world bounds (allPrimBounds), every other direction getBounds(d)
                const Range b = (fastKd && k < 3) ? Range{bmin[3 * (size_t)pn + k], bmax[3 * (size_t)pn + k]} : PrimBounds(bmin, bmax, tri9, isTri, pn, d);
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
                if (edgeT > db.min && edgeT < db.max) cands.push_back(Cand{k, i, nBelow, nAbove, edgeT});
                if (e[i].type == EdgeType::Start) ++nBelow;
            }
        }
        costs.resize(cands.size());
        if (fastKd) costsFixed.assign(cands.size(), std::numeric_limits<float>::infinity());
        const CostConsts cc{fastKd, invTotalSA, emptyBonus, isectCost, traversalCost, kdTraversalCost};
        auto costRange = [&](size_t k0, size_t k1, int w) {
            for (size_t k = k0; k < k1; ++k) {
                const Cand &c = cands[k];
                CostOne(cur, cc, &nodeDirs[3 * c.k], c.k < 3, c.nBelow, c.nAbove, c.t, scratch[(size_t)w], &candDirs[(size_t)w], &costs[k],
                        fastKd ? &costsFixed[k] : nullptr);
            }
        };
        // the costing hook (BspNodeParams::costFn): the node's candidates costed elsewhere, the flagged ones repaired here
        std::string hookErr;
        const HookResult hooked = RunCostHook(p, cands.size(), overflow, false, [&](BspNodeCostRequest &rq) {      // (secondsDevice: costFn alone)
            hookCands.resize(cands.size());
            for (size_t k = 0; k < cands.size(); ++k) hookCands[k] = bspnodecost::Cand{cands[k].k, cands[k].nBelow, cands[k].nAbove, cands[k].t};
            hookDirs.resize(nDirs);
            for (uint32_t k = 0; k < nDirs; ++k)
                hookDirs[k] = bspnodecost::SweepDir{{nodeDirs[3 * k], nodeDirs[3 * k + 1], nodeDirs[3 * k + 2]},
                                                    !fastKd ? bspnodecost::KIND_PLAIN : (k < 3 ? bspnodecost::KIND_KD_AXIS : bspnodecost::KIND_CHOSEN)};
            rq.mesh = reinterpret_cast<const kdopcost::Edge *>(cur.mesh.data()); rq.nEdges = (uint32_t)cur.mesh.size();
            rq.dirs = cur.dirs.data(); rq.M = (uint32_t)(cur.dirs.size() / 3);
            rq.sweep = hookDirs.data(); rq.nDirs = nDirs; rq.fastKd = fastKd;
            rq.sc = bspcost::Scalars{invTotalSA, emptyBonus, isectCost, traversalCost, kdTraversalCost, cur.nPrimitives, 0u, 0u, 0u, 0u};
            rq.cands = hookCands.data(); rq.n = cands.size();
            rq.costs = costs.data(); rq.costsFixed = fastKd ? costsFixed.data() : nullptr; rq.overflow = overflow.data();
            rq.level = maxDepth - cur.depth;
        }, [&](size_t k) {
            if (fastKd) costsFixed[k] = std::numeric_limits<float>::infinity();
            costRange(k, k + 1, 0);
        }, &hookErr);
        if (hooked == HookResult::Failed) return hookErr;
        if (hooked == HookResult::Costed) {
            // (costs[] and costsFixed[] are complete)
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
        // the reference's scan: strict `<`, so the first minimum in (direction, edge) order
        size_t best = (size_t)-1;
        float bestCost = std::numeric_limits<float>::infinity();
        for (size_t k = 0; k < cands.size(); ++k)
            if (costs[k] < bestCost) { bestCost = costs[k]; best = k; }

        if (fastKd) {
            // the second minimum (bestCostFixed / bestKFixed), over the chosen directions only; the leaf tests need both to fail
            size_t bestFixed = (size_t)-1;
            float bestCostFixed = std::numeric_limits<float>::infinity();
            for (size_t k = 0; k < cands.size(); ++k)
                if (cands[k].k >= 3 && costsFixed[k] < bestCostFixed) { bestCostFixed = costsFixed[k]; bestFixed = k; }
            if (bestCost > oldCost && bestCostFixed > oldCost) ++cur.badRefines;
            if ((bestCost > 4 * oldCost && bestCostFixed > 4 * oldCost && cur.nPrimitives < 16) || (best == (size_t)-1 && bestFixed == (size_t)-1) ||
                cur.badRefines == 3) {
                initLeaf(&prims[cur.primNums], cur.nPrimitives); ++nodeNum; continue;
            }
            // only the fixed minimum beat infinity: the reference classifies by edges[bestK = -1] (bspNodeBasedFastKd.cpp:274-284)
            if (best == (size_t)-1)
                return "every kd-aware candidate cost is infinite or NaN while a fixed-cost split exists: the reference's build is undefined there";
        } else {
            // Create leaf if no good splits were found
            if (bestCost > oldCost) ++cur.badRefines;
            if ((bestCost > 4 * oldCost && cur.nPrimitives < 16) || best == (size_t)-1 || cur.badRefines == 3) {
                initLeaf(&prims[cur.primNums], cur.nPrimitives); ++nodeNum; continue;
            }
        }

        // the winner's halves, measured (and so reoriented) as the scan left them
        const Cand win = cands[best];
        const float *winDir = &nodeDirs[3 * win.k];
        Scratch &s = scratch[0];
        std::vector<float> childDirs;
        float areaBelow, areaAbove;
        CutMeasure(cur, win.t, winDir, s, &childDirs, &areaBelow, &areaAbove);
        Mesh below = s.left, above = s.right;

        // Classify primitives with respect to split: prims1 first, in place, so that child 0's share does not overwrite it
        uint32_t n0 = 0, n1 = 0;
        const size_t prims1 = cur.primNums;
        const BoundEdge *e = edges[win.k].data();
        for (uint32_t i = win.i + 1; i < 2 * cur.nPrimitives; ++i)
            if (e[i].type == EdgeType::End) prims[prims1 + n1++] = e[i].primNum;
        const size_t prims0 = prims1 + n1;
        uint32_t nStart = 0;
        for (uint32_t i = 0; i < win.i; ++i) nStart += e[i].type == EdgeType::Start;
        if ((uint64_t)prims0 + nStart > primsCap)
            return "the build needs more than the reference's (maxDepth + 1) * N primitive slots; lower \"maxdepth\"";
        if (prims.size() < prims0 + nStart + 1) prims.resize(prims0 + nStart + 1);
        for (uint32_t i = 0; i < win.i; ++i)
            if (e[i].type == EdgeType::Start) prims[prims0 + n0++] = e[i].primNum;

        const bool axisNode = nFixed != 0 && win.k < 3;                // nbKdNodes / nbBSPNodes
        if (axisNode) ++t.axisNodes; else ++t.planeNodes;
        BspNode nd;                                    // treeInitInterior (BSP.h:32-37); BSPKdNode::initInteriorKd / initInterior (BSPKd.h:40-49)
        std::memcpy(&nd.a, &win.t, 4);
        nd.b = !fastKd ? 0u : (axisNode ? win.k : (uint32_t)BSPPAPERKD_PLANE);
        nodes.push_back(nd);
        if (fastKd && axisNode) t.axes.insert(t.axes.end(), 3, 0.f);   // a kd node holds no axis (the reference leaves it unset)
        else t.axes.insert(t.axes.end(), winDir, winDir + 3);
        stack.push_back(BuildNode{cur.depth - 1, n1, cur.badRefines, std::move(above), childDirs, areaAbove, prims1, nodeNum});
        stack.push_back(BuildNode{cur.depth - 1, n0, cur.badRefines, std::move(below), std::move(childDirs), areaBelow, prims0, (uint32_t)-1});
        ++nodeNum;
    }
    uint32_t depth = 0;
    (void)(fastKd ? CheckBspPaperKdTree(t, &depth) : CheckBspPaperTree(t, &depth));
    t.depth = depth;
    return "";
}

}  // namespace hprt
