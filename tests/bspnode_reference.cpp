// Test-side restatement of the fork's node-based BSP trees (accelerators/bspNodeBased.cpp, bspNodeBasedWithKd.cpp,
// bspNodeBasedFastKd.cpp, randomNormals.h, clustering.h): the three buildTree bodies and the three direction choosers, written
// independently of thesis-pbrt-v3_amd/csrc/ and in the reference's own shape — a single-threaded scan over the node's directions
// with running minima that keeps the best candidates' k-DOP halves, choosers over std::vector<V3> and std::set — where the library
// costs candidates in parallel and cuts the winner again.  The k-DOP with its own directions, PositiveX, getBounds, the build's
// working types, both node types and both walks are the general BSP trees' restatements' (tests/bsppaper_reference.cpp,
// tests/bsppaperkd_reference.cpp), which this file includes whole rather than repeat: the reference shares them too (BSP / BSPKd),
// and a node-based tree is walked by exactly those walks (their bspref_* / bspkdref_* entry points come along unused).
// The reference seeds std::mt19937 from std::random_device and cannot be reproduced; this restatement takes the seed the library
// takes and draws from the same <random> and libm ("parity unpinned").  Compiled with g++ at test time
// (tests/tree_ref.py through tests/bspnode_ref.py), driven through ctypes.
#include <random>
#include <set>
#include "bsppaperkd_reference.cpp"

namespace {

enum { ARBITRARY = 0, CLUSTER = 1, RANDOM = 2 };
enum { PLAIN = 0, WITHKD = 1, FASTKD = 2 };

struct OutOfRange {};      // a drawn index equal to np: the reference reads primNums[np]

// Triangle::Normal (shapes/triangle.cpp:584-594); Shape::Normal is (0, 0, 0)
V3 Normal(const Prim &pr) {
    if (!pr.tri) return V3(0, 0, 0);
    V3 n = Cross(pr.p[0] - pr.p[2], pr.p[1] - pr.p[2]);
    if (n.Length() > 0) n = Normalize(n);
    return n;
}
Float Angle(const V3 &v1, const V3 &v2) { return std::acos(std::max(std::min((Float)1.0, Dot(v1, v2)), (Float)-1.0)); }

// clustering.h:9-51
uint32_t calculateIdOfClosestMean(V3 &normal, const std::vector<V3> &means) {
    uint32_t closest = 0;
    Float closestAngle = Angle(normal, means[0]);
    for (uint32_t i = 1; i < means.size(); ++i) {
        Float currentAngle = Angle(normal, means[i]);
        if (currentAngle < closestAngle) { closest = i; closestAngle = currentAngle; }
    }
    return closest;
}
V3 calculateMeanVector(const std::vector<V3> &vectors) {
    if (vectors.empty()) return V3();
    V3 sumVector = V3();
    for (auto &vector : vectors) sumVector += vector;
    return Normalize(sumVector);
}
Float calculateMaxDifference(const std::vector<V3> &oldMeans, const std::vector<V3> &newMeans) {
    Float maxDiff = 0;
    for (uint32_t i = 0; i < oldMeans.size(); ++i) {
        V3 diff = oldMeans[i] - newMeans[i];
        maxDiff = std::max(maxDiff, Dot(diff, diff));
    }
    return maxDiff;
}
uint32_t random_int(std::mt19937 &gen, uint32_t from, uint32_t to) {
    std::uniform_real_distribution<> dis(from, to);
    const uint32_t r = uint32_t(dis(gen));
    if (r >= to) throw OutOfRange();
    return r;
}

// clustering.h:53-112
std::vector<V3> calculateClusterMeans(std::mt19937 &gen, const uint32_t K, const std::vector<Prim> &primitives, const uint32_t *primNums, const uint32_t np) {
    std::vector<V3> clusterMeans, newClusterMeans;
    std::vector<std::vector<V3>> clusters;
    std::vector<V3> normals;
    normals.reserve(np);
    for (uint32_t i = 0; i < np; ++i) normals.emplace_back(PositiveX(Normal(primitives[primNums[i]])));
    if (np <= K) return normals;
    std::set<uint32_t> nIds;
    while (nIds.size() < K) nIds.insert(random_int(gen, 0, np));
    for (auto &id : nIds) { clusterMeans.emplace_back(normals[id]); clusters.emplace_back(std::vector<V3>()); }
    newClusterMeans = clusterMeans;
    const uint32_t maxIterations = 500;
    uint32_t iterations = 0;
    while (iterations < maxIterations && (iterations == 0 || calculateMaxDifference(clusterMeans, newClusterMeans) > 0.000001)) {
        ++iterations;
        clusterMeans = newClusterMeans;
        for (auto &n : normals) clusters[calculateIdOfClosestMean(n, clusterMeans)].emplace_back(n);
        for (uint32_t i = 0; i < K; ++i) {
            if (clusters[i].empty()) {
                std::set<uint32_t> nIds;
                while (nIds.size() < K) nIds.insert(random_int(gen, 0, np));
                std::vector<uint32_t> v(nIds.begin(), nIds.end());
                for (uint32_t ii = 0; ii < K; ++ii) {
                    auto id = v[ii];
                    newClusterMeans[ii] = normals[id];
                    clusters[ii].clear();
                }
                break;
            }
            newClusterMeans[i] = calculateMeanVector(clusters[i]);
            clusters[i].clear();
        }
    }
    return newClusterMeans;
}
// randomNormals.h:13-46
std::vector<V3> chooseArbitraryNormals(std::mt19937 &gen, const uint32_t K, const std::vector<Prim> &primitives, const uint32_t *primNums, const uint32_t np) {
    std::set<uint32_t> nIds;
    std::vector<V3> arbitraryNormals;
    while (nIds.size() < std::min(np, K)) nIds.insert(random_int(gen, 0, np));
    arbitraryNormals.reserve(nIds.size());
    for (auto &id : nIds) arbitraryNormals.emplace_back(PositiveX(Normal(primitives[primNums[id]])));
    return arbitraryNormals;
}
std::vector<V3> chooseRandomDirections(std::mt19937 &gen, const uint32_t K) {
    const Float Pi = 3.14159265358979323846;
    std::uniform_real_distribution<> disPhi(0, 2 * Pi);
    std::uniform_real_distribution<> disCosTheta(-1, 1);
    std::vector<V3> randomDirections;
    for (uint32_t i = 0; i < K; i++) {
        Float phi = disPhi(gen);
        Float cosTheta = disCosTheta(gen);
        Float theta = std::acos(cosTheta);
        Float x = std::sin(theta) * std::cos(phi);
        Float y = std::sin(theta) * std::sin(phi);
        Float z = std::cos(theta);
        randomDirections.emplace_back(PositiveX(V3(x, y, z)));
    }
    return randomDirections;
}
std::vector<V3> calculateDirections(int chooser, std::mt19937 &gen, uint32_t K, const std::vector<Prim> &primitives, const uint32_t *primNums, uint32_t np) {
    if (chooser == ARBITRARY) return chooseArbitraryNormals(gen, K, primitives, primNums, np);
    if (chooser == RANDOM) return chooseRandomDirections(gen, K);
    return calculateClusterMeans(gen, K, primitives, primNums, np);
}

DMesh RootMesh(const B3 &b) {
    DMesh root;
    V3 v1 = b.pMin, v2(b.pMin.x, b.pMin.y, b.pMax.z), v3(b.pMin.x, b.pMax.y, b.pMin.z), v4(b.pMax.x, b.pMin.y, b.pMin.z);
    V3 v5(b.pMin.x, b.pMax.y, b.pMax.z), v6(b.pMax.x, b.pMin.y, b.pMax.z), v7(b.pMax.x, b.pMax.y, b.pMin.z), v8 = b.pMax;
    root.edges = {{v1, v2, 1, 3}, {v1, v3, 1, 5}, {v1, v4, 3, 5}, {v2, v5, 1, 4}, {v2, v6, 3, 4}, {v3, v5, 1, 2},
                  {v3, v7, 2, 5}, {v4, v6, 0, 3}, {v4, v7, 0, 5}, {v5, v8, 2, 4}, {v6, v8, 0, 4}, {v7, v8, 0, 2}};
    root.directions = {V3(1, 0, 0), V3(0, 1, 0), V3(0, 0, 1)};
    return root;
}
uint32_t MaxDepth(uint32_t maxDepth, size_t N) {
    if (maxDepth != (uint32_t)-1) return maxDepth;
    const int lg = N ? 63 - __builtin_clzll((uint64_t)N) : -1;
    return (uint32_t)std::round(2 + 1.6f * lg);
}
bool EdgeLess(const BoundEdge &e0, const BoundEdge &e1) {
    if (e0.t == e1.t) return (int)e0.type < (int)e1.type;
    else return e0.t < e1.t;
}

// BSPNodeBased::buildTree (bspNodeBased.cpp:27-223); withKd: BSPNodeBasedWithKd::buildTree
void BuildNodeBased(const std::vector<Prim> &prims, int chooser, bool withKd, uint32_t K, uint32_t seed, uint32_t isectCost, uint32_t traversalCost,
                    Float emptyBonus, uint32_t maxPrims, uint32_t maxDepth, Tree *tree) {
    std::mt19937 gen(seed);
    const size_t N = prims.size();
    maxDepth = MaxDepth(maxDepth, N);
    tree->bounds = B3();
    for (const Prim &p : prims) tree->bounds = Union(tree->bounds, p.wb);
    DMesh root = RootMesh(tree->bounds);
    std::vector<std::vector<BoundEdge>> edges(K, std::vector<BoundEdge>(2 * N));
    std::vector<uint32_t> primsBuf((size_t)(maxDepth + 1) * N + 1);
    for (uint32_t i = 0; i < N; ++i) primsBuf[i] = i;
    std::vector<BSPNode> &nodes = tree->nodes;
    auto InitLeaf = [&](uint32_t nodeNum, uint32_t *primNums, uint32_t np) {
        nodes[nodeNum].flags = 1u;
        nodes[nodeNum].nPrims |= (np << 1u);
        if (np == 0) nodes[nodeNum].onePrimitive = 0;
        else if (np == 1) nodes[nodeNum].onePrimitive = primNums[0];
        else {
            nodes[nodeNum].primitiveIndicesOffset = (uint32_t)tree->primitiveIndices.size();
            for (uint32_t i = 0; i < np; ++i) tree->primitiveIndices.push_back(primNums[i]);
        }
    };
    uint32_t nodeNum = 0;
    std::vector<BuildNode> stack;
    const Float rootArea = root.SurfaceArea();
    stack.push_back(BuildNode{maxDepth, (uint32_t)N, 0, root, rootArea, &primsBuf[0], (uint32_t)-1});
    while (!stack.empty()) {
        BuildNode cur = stack.back();
        stack.pop_back();
        if (cur.parentNum != (uint32_t)-1) nodes[cur.parentNum].aboveChild |= (nodeNum << 1u);
        nodes.emplace_back();
        memset(&nodes.back(), 0, sizeof(BSPNode));
        if (cur.nPrimitives <= maxPrims || cur.depth == 0) { InitLeaf(nodeNum++, cur.primNums, cur.nPrimitives); continue; }
        uint32_t bestK = (uint32_t)-1, bestOffset = (uint32_t)-1;
        std::pair<DMesh, DMesh> best;
        std::pair<Float, Float> bestAreas(0, 0);
        Float bestCost = Infinity;
        const Float oldCost = isectCost * Float(cur.nPrimitives);
        const Float invTotalSA = 1 / cur.area;
        std::vector<V3> nodeDirections;
        if (!withKd) nodeDirections = calculateDirections(chooser, gen, K, prims, cur.primNums, cur.nPrimitives);
        else {
            const uint32_t Kmeans = K - 3;
            nodeDirections.emplace_back(1, 0, 0);
            nodeDirections.emplace_back(0, 1, 0);
            nodeDirections.emplace_back(0, 0, 1);
            if (Kmeans > 0) {
                auto generated = calculateDirections(chooser, gen, Kmeans, prims, cur.primNums, cur.nPrimitives);
                nodeDirections.insert(nodeDirections.end(), generated.begin(), generated.end());
            }
        }
        for (uint32_t k = 0; k < nodeDirections.size(); ++k) {
            V3 d = nodeDirections[k];
            Bnds db;
            for (auto &e : cur.mesh.edges) db = Union(db, e.getBounds(d));
            for (uint32_t i = 0; i < cur.nPrimitives; ++i) {
                const uint32_t pn = cur.primNums[i];
                const Bnds b = GetBounds(prims[pn], d);
                edges[k][2 * i] = BoundEdge{b.min, pn, EdgeType::Start};
                edges[k][2 * i + 1] = BoundEdge{b.max, pn, EdgeType::End};
            }
            std::sort(&edges[k][0], &edges[k][0] + 2 * cur.nPrimitives, EdgeLess);
            uint32_t nBelow = 0, nAbove = cur.nPrimitives;
            for (uint32_t i = 0; i < 2 * cur.nPrimitives; ++i) {
                if (edges[k][i].type == EdgeType::End) --nAbove;
                const Float edgeT = edges[k][i].t;
                if (edgeT > db.min && edgeT < db.max) {
                    std::pair<DMesh, DMesh> cut = cur.mesh.cut(edgeT, d);
                    const Float areaBelow = cut.first.SurfaceArea(), areaAbove = cut.second.SurfaceArea();
                    const Float pBelow = areaBelow * invTotalSA, pAbove = areaAbove * invTotalSA;
                    const Float eb = (nAbove == 0 || nBelow == 0) ? emptyBonus : 0;
                    const Float cost = traversalCost + isectCost * (1 - eb) * (pBelow * nBelow + pAbove * nAbove);
                    if (cost < bestCost) { bestCost = cost; bestK = k; bestOffset = i; best = cut; bestAreas = std::make_pair(areaBelow, areaAbove); }
                }
                if (edges[k][i].type == EdgeType::Start) ++nBelow;
            }
        }
        if (bestCost > oldCost) ++cur.badRefines;
        if ((bestCost > 4 * oldCost && cur.nPrimitives < 16) || bestK == (uint32_t)-1 || cur.badRefines == 3) {
            InitLeaf(nodeNum++, cur.primNums, cur.nPrimitives);
            continue;
        }
        uint32_t n0 = 0, n1 = 0;
        uint32_t *prims1 = cur.primNums;
        for (uint32_t i = bestOffset + 1; i < 2 * cur.nPrimitives; ++i)
            if (edges[bestK][i].type == EdgeType::End) prims1[n1++] = edges[bestK][i].primNum;
        uint32_t *prims0 = prims1 + n1;
        for (uint32_t i = 0; i < bestOffset; ++i)
            if (edges[bestK][i].type == EdgeType::Start) prims0[n0++] = edges[bestK][i].primNum;
        const Float tSplit = edges[bestK][bestOffset].t;
        const V3 axis = nodeDirections[bestK];          // treeInitInterior (BSP.h:32-37)
        nodes[nodeNum].split = tSplit;
        nodes[nodeNum].splitAxis[0] = axis.x; nodes[nodeNum].splitAxis[1] = axis.y; nodes[nodeNum].splitAxis[2] = axis.z;
        nodes[nodeNum].flags = 0;
        stack.push_back(BuildNode{cur.depth - 1, n1, cur.badRefines, best.second, bestAreas.second, prims1, nodeNum});
        stack.push_back(BuildNode{cur.depth - 1, n0, cur.badRefines, best.first, bestAreas.first, prims0, (uint32_t)-1});
        ++nodeNum;
    }
}

struct Undefined {};       // bestK == -1 && bestKFixed != -1: the reference classifies by edges[-1]

// BSPNodeBasedFastKd::buildTree (bspNodeBasedFastKd.cpp:28-330)
void BuildFastKd(const std::vector<Prim> &prims, int chooser, uint32_t K, uint32_t seed, uint32_t isectCost, uint32_t traversalCost,
                 uint32_t kdTraversalCost, Float emptyBonus, uint32_t maxPrims, uint32_t maxDepth, KdAwareTree *tree) {
    const Float BSP_ALPHA = 0.1;
    std::mt19937 gen(seed);
    const size_t N = prims.size();
    maxDepth = MaxDepth(maxDepth, N);
    tree->bounds = B3();
    for (const Prim &p : prims) tree->bounds = Union(tree->bounds, p.wb);
    DMesh root = RootMesh(tree->bounds);
    const V3 kdDirections[3] = {V3(1, 0, 0), V3(0, 1, 0), V3(0, 0, 1)};
    std::vector<std::vector<BoundEdge>> edges(K, std::vector<BoundEdge>(2 * N));
    std::vector<uint32_t> primsBuf((size_t)(maxDepth + 1) * N + 1);
    for (uint32_t i = 0; i < N; ++i) primsBuf[i] = i;
    std::vector<BSPKdNode> &nodes = tree->nodes;
    auto InitLeaf = [&](uint32_t nodeNum, uint32_t *primNums, uint32_t np) {     // BSPKd.h:21-34
        nodes[nodeNum].flags = 3u;
        nodes[nodeNum].nPrims |= (np << 3u);
        if (np == 0) nodes[nodeNum].onePrimitive = 0;
        else if (np == 1) nodes[nodeNum].onePrimitive = primNums[0];
        else {
            nodes[nodeNum].primitiveIndicesOffset = (uint32_t)tree->primitiveIndices.size();
            for (uint32_t i = 0; i < np; ++i) tree->primitiveIndices.push_back(primNums[i]);
        }
    };
    uint32_t nodeNum = 0;
    std::vector<BuildNode> stack;
    const Float rootArea = root.SurfaceArea();
    stack.push_back(BuildNode{maxDepth, (uint32_t)N, 0, root, rootArea, &primsBuf[0], (uint32_t)-1});
    while (!stack.empty()) {
        BuildNode cur = stack.back();
        stack.pop_back();
        if (cur.parentNum != (uint32_t)-1) nodes[cur.parentNum].aboveChild |= (nodeNum << 3u);
        nodes.emplace_back();
        memset(&nodes.back(), 0, sizeof(BSPKdNode));
        if (cur.nPrimitives <= maxPrims || cur.depth == 0) { InitLeaf(nodeNum++, cur.primNums, cur.nPrimitives); continue; }
        uint32_t bestK = (uint32_t)-1, bestOffset = (uint32_t)-1, bestKFixed = (uint32_t)-1, bestOffsetFixed = (uint32_t)-1;
        std::pair<DMesh, DMesh> best, bestFixed;
        std::pair<Float, Float> bestAreas(0, 0), bestAreasFixed(0, 0);
        Float bestCost = Infinity, bestCostFixed = Infinity;
        const Float oldCost = isectCost * Float(cur.nPrimitives);
        const Float invTotalSA = 1 / cur.area;
        // Sweep for kd directions
        for (uint32_t k = 0; k < 3; ++k) {
            V3 d = kdDirections[k];
            Bnds db;
            for (auto &e : cur.mesh.edges) db = Union(db, e.getBounds(d));
            for (uint32_t i = 0; i < cur.nPrimitives; ++i) {
                const uint32_t pn = cur.primNums[i];
                edges[k][2 * i] = BoundEdge{prims[pn].wb.pMin[k], pn, EdgeType::Start};
                edges[k][2 * i + 1] = BoundEdge{prims[pn].wb.pMax[k], pn, EdgeType::End};
            }
            std::sort(&edges[k][0], &edges[k][0] + 2 * cur.nPrimitives, EdgeLess);
            uint32_t nBelow = 0, nAbove = cur.nPrimitives;
            for (uint32_t i = 0; i < 2 * cur.nPrimitives; ++i) {
                if (edges[k][i].type == EdgeType::End) --nAbove;
                const Float edgeT = edges[k][i].t;
                if (edgeT > db.min && edgeT < db.max) {
                    std::pair<DMesh, DMesh> cut = cur.mesh.cut(edgeT, d);
                    const Float areaBelow = cut.first.SurfaceArea(), areaAbove = cut.second.SurfaceArea();
                    const Float pBelow = areaBelow * invTotalSA, pAbove = areaAbove * invTotalSA;
                    const Float eb = (nAbove == 0 || nBelow == 0) ? emptyBonus : 0;
                    const Float cost = kdTraversalCost + isectCost * (1 - eb) * (pBelow * nBelow + pAbove * nAbove);
                    if (cost < bestCost) { bestCost = cost; bestK = k; bestOffset = i; best = cut; bestAreas = std::make_pair(areaBelow, areaAbove); }
                }
                if (edges[k][i].type == EdgeType::Start) ++nBelow;
            }
        }
        const uint32_t Kmeans = K - 3;
        std::vector<V3> nodeDirections;
        if (Kmeans > 0) {
            auto generated = calculateDirections(chooser, gen, Kmeans, prims, cur.primNums, cur.nPrimitives);
            nodeDirections.insert(nodeDirections.end(), generated.begin(), generated.end());
        }
        for (uint32_t k = 0; k < nodeDirections.size(); ++k) {
            V3 d = nodeDirections[k];
            const uint32_t edgeK = k + 3;
            Bnds db;
            for (auto &e : cur.mesh.edges) db = Union(db, e.getBounds(d));
            for (uint32_t i = 0; i < cur.nPrimitives; ++i) {
                const uint32_t pn = cur.primNums[i];
                const Bnds b = GetBounds(prims[pn], d);
                edges[edgeK][2 * i] = BoundEdge{b.min, pn, EdgeType::Start};
                edges[edgeK][2 * i + 1] = BoundEdge{b.max, pn, EdgeType::End};
            }
            std::sort(&edges[edgeK][0], &edges[edgeK][0] + 2 * cur.nPrimitives, EdgeLess);
            uint32_t nBelow = 0, nAbove = cur.nPrimitives;
            for (uint32_t i = 0; i < 2 * cur.nPrimitives; ++i) {
                if (edges[edgeK][i].type == EdgeType::End) --nAbove;
                const Float edgeT = edges[edgeK][i].t;
                if (edgeT > db.min && edgeT < db.max) {
                    std::pair<DMesh, DMesh> cut = cur.mesh.cut(edgeT, d);
                    const Float areaBelow = cut.first.SurfaceArea(), areaAbove = cut.second.SurfaceArea();
                    const Float pBelow = areaBelow * invTotalSA, pAbove = areaAbove * invTotalSA;
                    const Float eb = (nAbove == 0 || nBelow == 0) ? emptyBonus : 0;
                    const Float costIntersection = isectCost * (1 - eb) * (pBelow * nBelow + pAbove * nAbove);
                    const Float costFixed = traversalCost + costIntersection;
                    const Float cost = BSP_ALPHA * isectCost * (cur.nPrimitives - 1) + kdTraversalCost + costIntersection;
                    if (cost < bestCost) { bestCost = cost; bestK = edgeK; bestOffset = i; best = cut; bestAreas = std::make_pair(areaBelow, areaAbove); }
                    if (costFixed < bestCostFixed) {
                        bestCostFixed = costFixed; bestKFixed = edgeK; bestOffsetFixed = i; bestFixed = cut;
                        bestAreasFixed = std::make_pair(areaBelow, areaAbove);
                    }
                }
                if (edges[edgeK][i].type == EdgeType::Start) ++nBelow;
            }
        }
        if (bestCost > oldCost && bestCostFixed > oldCost) ++cur.badRefines;
        if ((bestCost > 4 * oldCost && bestCostFixed > 4 * oldCost && cur.nPrimitives < 16) || (bestK == (uint32_t)-1 && bestKFixed == (uint32_t)-1) ||
            cur.badRefines == 3) {
            InitLeaf(nodeNum++, cur.primNums, cur.nPrimitives);
            continue;
        }
        if (bestK == (uint32_t)-1) throw Undefined();
        (void)bestOffsetFixed; (void)bestFixed; (void)bestAreasFixed;
        uint32_t n0 = 0, n1 = 0;
        uint32_t *prims1 = cur.primNums;
        for (uint32_t i = bestOffset + 1; i < 2 * cur.nPrimitives; ++i)
            if (edges[bestK][i].type == EdgeType::End) prims1[n1++] = edges[bestK][i].primNum;
        uint32_t *prims0 = prims1 + n1;
        for (uint32_t i = 0; i < bestOffset; ++i)
            if (edges[bestK][i].type == EdgeType::Start) prims0[n0++] = edges[bestK][i].primNum;
        const Float tSplit = edges[bestK][bestOffset].t;
        nodes[nodeNum].split = tSplit;
        if (bestK < 3) nodes[nodeNum].flags = bestK;                       // initInteriorKd: splitAxis stays unset (here zero)
        else {                                                             // initInterior (BSPKd.h:40-44)
            const V3 axis = nodeDirections[bestK - 3];
            nodes[nodeNum].splitAxis[0] = axis.x; nodes[nodeNum].splitAxis[1] = axis.y; nodes[nodeNum].splitAxis[2] = axis.z;
            nodes[nodeNum].flags = 4;
        }
        stack.push_back(BuildNode{cur.depth - 1, n1, cur.badRefines, best.second, bestAreas.second, prims1, nodeNum});
        stack.push_back(BuildNode{cur.depth - 1, n0, cur.badRefines, best.first, bestAreas.first, prims0, (uint32_t)-1});
        ++nodeNum;
    }
}

// form FASTKD builds *kd, the others *plain; false (g_err) where the reference's build is undefined
bool BuildForm(const std::vector<Prim> &prims, int chooser, int form, uint32_t K, uint32_t seed, uint32_t isectCost, uint32_t travCost, uint32_t kdTravCost,
               Float emptyBonus, uint32_t maxPrims, uint32_t maxDepth, Tree *plain, KdAwareTree *kd) {
    if (form != PLAIN && K < 3) { g_err = "K < 3: K - 3 wraps"; return false; }
    try {
        if (form == FASTKD) BuildFastKd(prims, chooser, K, seed, isectCost, travCost, kdTravCost, emptyBonus, maxPrims, maxDepth, kd);
        else BuildNodeBased(prims, chooser, form == WITHKD, K, seed, isectCost, travCost, emptyBonus, maxPrims, maxDepth, plain);
    } catch (const OutOfRange &) { g_err = "a drawn index equals np"; return false; }
    catch (const Undefined &) { g_err = "bestK == -1 && bestKFixed != -1"; return false; }
    return true;
}

// what the entry points hand out: the form says which of the two tree / scene types is behind the pointer
struct BuiltTree { int form; Tree plain; KdAwareTree kd; };
struct BuiltScene { int form; BspScene *plain; BspKdScene *kd; };

}  // namespace

extern "C" {

const char *bspnoderef_last_error() { return g_err.c_str(); }

// build over n triangles (9 floats each, creation order); sizes[0..1] = nodes, primitiveIndices entries; null (last_error) where
// the reference's build is undefined
void *bspnoderef_build(size_t n, const float *p9, int chooser, int form, int K, uint32_t seed, int isectCost, int travCost, int kdTravCost, float emptyBonus,
                       int maxPrims, int maxDepth, uint32_t sizes[2]) {
    BuiltTree *t = new BuiltTree();
    t->form = form;
    if (!BuildForm(TrianglePrims(n, p9), chooser, form, (uint32_t)K, seed, (uint32_t)isectCost, (uint32_t)travCost, (uint32_t)kdTravCost, emptyBonus,
                   (uint32_t)maxPrims, (uint32_t)maxDepth, &t->plain, &t->kd)) { delete t; return nullptr; }
    sizes[0] = (uint32_t)(form == FASTKD ? t->kd.nodes.size() : t->plain.nodes.size());
    sizes[1] = (uint32_t)(form == FASTKD ? t->kd.primitiveIndices.size() : t->plain.primitiveIndices.size());
    return t;
}
// nodes20: 5 words per node (the axis words of leaves and of fastkd's kd nodes zero)
void bspnoderef_copy(void *h, void *nodes20, uint32_t *idx) {
    const BuiltTree *t = (const BuiltTree *)h;
    if (t->form == FASTKD) CopyTree(t->kd, nodes20, idx, nullptr);
    else CopyTree(t->plain, nodes20, idx, nullptr);
}
void bspnoderef_free(void *h) { delete (BuiltTree *)h; }

// `draws` calls of a chooser over the n triangles (all of them the node's primitives, in order) from one engine; counts[k] =
// directions of call k, dirs their components in order.  Returns 0, or 1 (last_error) where a drawn index equals n.
int bspnoderef_choose(int chooser, uint32_t K, uint32_t seed, size_t n, const float *p9, uint32_t draws, uint32_t *counts, float *dirs) {
    const std::vector<Prim> prims = TrianglePrims(n, p9);
    std::vector<uint32_t> primNums(n);
    for (size_t i = 0; i < n; ++i) primNums[i] = (uint32_t)i;
    std::mt19937 gen(seed);
    size_t w = 0;
    try {
        for (uint32_t k = 0; k < draws; ++k) {
            const std::vector<V3> d = calculateDirections(chooser, gen, K, prims, primNums.data(), (uint32_t)n);
            counts[k] = (uint32_t)d.size();
            for (const V3 &v : d) { dirs[w++] = v.x; dirs[w++] = v.y; dirs[w++] = v.z; }
        }
    } catch (const OutOfRange &) { g_err = "a drawn index equals np"; return 1; }
    return 0;
}
// the index sets `while (nIds.size() < count) nIds.insert(random_int(gen, 0, np))` draws, `draws` of them from one engine:
// ids[count * k ..] in set order
int bspnoderef_draw_ids(uint32_t count, uint32_t np, uint32_t seed, uint32_t draws, uint32_t *ids) {
    std::mt19937 gen(seed);
    try {
        for (uint32_t k = 0; k < draws; ++k) {
            std::set<uint32_t> nIds;
            while (nIds.size() < count) nIds.insert(random_int(gen, 0, np));
            for (uint32_t id : nIds) *ids++ = id;
        }
    } catch (const OutOfRange &) { g_err = "a drawn index equals np"; return 1; }
    return 0;
}

// a baked scene (no instances), its BVH and the restated tree of (chooser, form, K, seed) with the default parameters, walked by
// BSP::Intersect / IntersectP (plain, withkd) or BSPKd::Intersect / IntersectP (fastkd; five counter columns)
void *bspnoderef_scene_load(const char *path, int chooser, int form, int K, uint32_t seed) {
    BuiltScene *s = new BuiltScene{form, nullptr, nullptr};
    bool ok;
    if (form == FASTKD) {
        s->kd = LoadSceneRef<BspKdStep>(path);
        ok = s->kd && BuildForm(s->kd->Prims(), chooser, form, (uint32_t)K, seed, 80, 5, 1, 0.f, 1, (uint32_t)-1, nullptr, &s->kd->tree);
    } else {
        s->plain = LoadSceneRef<BspStep>(path);
        ok = s->plain && BuildForm(s->plain->Prims(), chooser, form, (uint32_t)K, seed, 80, 5, 1, 0.f, 1, (uint32_t)-1, &s->plain->tree, nullptr);
    }
    if (!ok) { delete s->plain; delete s->kd; delete s; return nullptr; }
    return s;
}
size_t bspnoderef_scene_max_todo(void *h, uint32_t *out) { const BuiltScene *s = (const BuiltScene *)h; return s->kd ? SceneMaxTodo(s->kd, out) : SceneMaxTodo(s->plain, out); }
void bspnoderef_scene_free(void *h) { BuiltScene *s = (BuiltScene *)h; delete s->plain; delete s->kd; delete s; }
size_t bspnoderef_scene_prims(void *h) { const BuiltScene *s = (const BuiltScene *)h; return s->kd ? s->kd->scene.prims.size() : s->plain->scene.prims.size(); }
size_t bspnoderef_scene_triangles(void *h, float *p9) { const BuiltScene *s = (const BuiltScene *)h; return s->kd ? SceneTriangles(s->kd, p9) : SceneTriangles(s->plain, p9); }
void bspnoderef_scene_tree(void *h, uint32_t sizes[2], void *nodes20, uint32_t *idx) {
    const BuiltScene *s = (const BuiltScene *)h;
    if (s->kd) SceneTree(s->kd, sizes, nodes20, idx); else SceneTree(s->plain, sizes, nodes20, idx);
}
// counters: 5 columns for a fastkd scene (the fifth the kd interior nodes), else 4
void bspnoderef_intersect(void *h, size_t n, const float *o, const float *d, const float *tmax, float *tOut, int32_t *primOut, float *bary, uint64_t *counters) {
    const BuiltScene *s = (const BuiltScene *)h;
    if (s->kd) IntersectRays(s->kd, n, o, d, tmax, tOut, primOut, bary, counters, 5);
    else IntersectRays(s->plain, n, o, d, tmax, tOut, primOut, bary, counters, 4);
}
void bspnoderef_occluded(void *h, size_t n, const float *o, const float *d, const float *tmax, uint8_t *occ, uint64_t *counters) {
    const BuiltScene *s = (const BuiltScene *)h;
    if (s->kd) OccludedRays(s->kd, n, o, d, tmax, occ, counters, 5);
    else OccludedRays(s->plain, n, o, d, tmax, occ, counters, 4);
}

}  // extern "C"
