// Test-side restatement of the fork's kd-aware RBSP tree (accelerators/rbspKd.cpp with kDOPMesh.h, RBSPShared.h):
// RBSPKd::buildTree and the two walks, Intersect and IntersectP, written independently of thesis-pbrt-v3_amd/csrc/ over the
// oracle's vector type and primitive tests (oracle/orc_accel.h, included read-only).  It follows the reference's own shape — a
// single-threaded scan with two running minima that keeps the best candidate's k-DOP halves — where the library costs candidates
// in parallel and cuts the winner again.  The walks count kd (direction < 3) and bsp interior nodes apart, and can be switched to
// the dot-product step of every node (RBSP's), the control that shows which rays tell the two interior forms apart.  Compiled
// with g++ at test time (tests/rbspkd_ref.py), driven through ctypes.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <utility>
#include <vector>
#include "orc_accel.h"

namespace orc { bool g_use_libm = false; }
using namespace orc;

namespace {

struct Node {                       // RBSPNode: union { split, onePrimitive, primitiveIndicesOffset }; union { flags, nPrims, aboveChild }
    union { float split; uint32_t onePrimitive; uint32_t primitiveIndicesOffset; };
    union { uint32_t flags; uint32_t nPrims; uint32_t aboveChild; };
};
static_assert(sizeof(Node) == 8, "RBSPNode is 8 bytes");

uint32_t BitOffset(uint32_t M) { return sizeof(uint32_t) * 8 - __builtin_clz(M + 1 - 1); }   // log2_fast(M + 1)
uint32_t BitMask(uint32_t M) { return (1u << BitOffset(M)) - 1; }

struct Bnds { Float min = std::numeric_limits<Float>::max(), max = std::numeric_limits<Float>::lowest(); };
Bnds Union(const Bnds &a, const Bnds &b) { Bnds r; r.min = std::min(a.min, b.min); r.max = std::max(a.max, b.max); return r; }

struct KEdge {
    V3 v1, v2; uint32_t faceId1, faceId2;
    Bnds getBounds(const V3 &d) const { Bnds b; const Float t1 = Dot(d, v1), t2 = Dot(d, v2); b.max = std::max(t1, t2); b.min = std::min(t1, t2); return b; }
};
struct KMesh { std::vector<KEdge> edges; };

void AddIfNeeded(KMesh &m, const KEdge &e) {
    for (auto &x : m.edges) if ((x.v1 == e.v2 && x.v2 == e.v1) || (x.v1 == e.v1 && x.v2 == e.v2)) return;
    m.edges.push_back(e);
}
void Helper(std::vector<V3> &pts, const V3 &p) { if (std::find(pts.begin(), pts.end(), p) == pts.end()) pts.push_back(p); }

void AddEdge(KMesh &left, KMesh &right, KEdge edge, std::vector<KEdge> &coincident, std::vector<std::vector<V3>> &fv, Float t, Float t1, Float t2) {
    V3 d = edge.v2 - edge.v1;
    if (t1 < t && t2 < t) left.edges.push_back(edge);
    else if (t1 > t && t2 > t) right.edges.push_back(edge);
    else if (t1 < t && t == t2) { left.edges.push_back(edge); Helper(fv[edge.faceId1], edge.v2); Helper(fv[edge.faceId2], edge.v2); }
    else if (t1 == t && t < t2) { right.edges.push_back(edge); Helper(fv[edge.faceId1], edge.v1); Helper(fv[edge.faceId2], edge.v1); }
    else if (t1 < t && t < t2) {
        Float tAlongEdge = (-(t1 - t)) / (t2 - t1);
        V3 vs(edge.v1 + tAlongEdge * d);
        left.edges.push_back(KEdge{edge.v1, vs, edge.faceId1, edge.faceId2});
        right.edges.push_back(KEdge{vs, edge.v2, edge.faceId1, edge.faceId2});
        Helper(fv[edge.faceId1], vs); Helper(fv[edge.faceId2], vs);
    } else if (t1 == t && t == t2) coincident.push_back(edge);
}

std::pair<KMesh, KMesh> CutMesh(const std::vector<KEdge> &edges, uint32_t M, Float t, const V3 &direction, uint32_t dId) {
    KMesh left, right;
    std::vector<std::vector<V3>> fv(2 * M);
    std::vector<KEdge> coincident;
    for (auto &edge : edges) {
        Float t1 = Dot(direction, edge.v1), t2 = Dot(direction, edge.v2);
        if (t1 > t2) AddEdge(left, right, KEdge{edge.v2, edge.v1, edge.faceId1, edge.faceId2}, coincident, fv, t, t2, t1);
        else AddEdge(left, right, edge, coincident, fv, t, t1, t2);
    }
    for (auto &edge : coincident) {
        for (auto &le : left.edges) {
            if (le.faceId1 == edge.faceId1 || le.faceId2 == edge.faceId1) {
                left.edges.push_back(KEdge{edge.v1, edge.v2, edge.faceId1, 2 * dId});
                right.edges.push_back(KEdge{edge.v1, edge.v2, edge.faceId2, 2 * dId + 1});
                break;
            } else if (le.faceId1 == edge.faceId2 || le.faceId2 == edge.faceId2) {
                left.edges.push_back(KEdge{edge.v1, edge.v2, edge.faceId2, 2 * dId});
                right.edges.push_back(KEdge{edge.v1, edge.v2, edge.faceId1, 2 * dId + 1});
                break;
            }
        }
    }
    for (uint32_t i = 0; i < 2 * M; ++i)
        if (fv[i].size() == 2) {
            AddIfNeeded(left, KEdge{fv[i][0], fv[i][1], i, 2 * dId});
            AddIfNeeded(right, KEdge{fv[i][0], fv[i][1], i, 2 * dId + 1});
        }
    return std::make_pair(left, right);
}

Float MeshArea(std::vector<KEdge> &edges, const std::vector<V3> &dirs) {
    std::vector<std::vector<KEdge *>> faces(2 * dirs.size());
    for (auto &e : edges) { faces[e.faceId1].push_back(&e); faces[e.faceId2].push_back(&e); }
    Float SA = 0;
    for (uint32_t i = 0; i < 2 * dirs.size(); ++i) {
        V3 FSA;
        const std::vector<KEdge *> &face = faces[i];
        if (!face.empty()) {
            std::vector<bool> used(face.size(), false);
            uint32_t edgeId = 0;
            do {
                if (used[edgeId]) break;
                used[edgeId] = true;
                KEdge *cur = face[edgeId];
                FSA += Cross(cur->v1, cur->v2);
                for (uint32_t j = 0; j < face.size(); ++j) {
                    if (j == edgeId) continue;
                    if (face[j]->v2 == cur->v2) std::swap(face[j]->v1, face[j]->v2);
                    if (face[j]->v1 == cur->v2 && !used[j]) { edgeId = j; break; }
                }
            } while (edgeId != 0);
        }
        SA += std::abs(Dot(dirs[i / 2], FSA));
    }
    return SA / 2.0f;
}

std::vector<V3> Directions(uint32_t N) {
    std::vector<V3> d;
    auto nz = [](V3 v) { return v / v.Length(); };
    d.push_back(V3(1.0, 0.0, 0.0)); d.push_back(V3(0.0, 1.0, 0.0)); d.push_back(V3(0.0, 0.0, 1.0));
    if (N == 7 || N == 13) { d.push_back(nz(V3(1, 1, 1))); d.push_back(nz(V3(1, -1, 1))); d.push_back(nz(V3(1, 1, -1))); d.push_back(nz(V3(1, -1, -1))); }
    if (N == 9 || N == 13) {
        d.push_back(nz(V3(1, 1, 0))); d.push_back(nz(V3(1, 0, 1))); d.push_back(nz(V3(0, 1, 1)));
        d.push_back(nz(V3(1, -1, 0))); d.push_back(nz(V3(1, 0, -1))); d.push_back(nz(V3(0, 1, -1)));
    }
    return d;
}

// A primitive as the builder sees it: a triangle's three world vertices, or (tri == false) a world bound
struct Prim { bool tri; V3 p[3]; B3 wb; };

struct Tree {
    uint32_t M = 3;
    std::vector<V3> dirs;
    std::vector<Node> nodes;
    std::vector<uint32_t> primitiveIndices;
    B3 bounds;
};

enum class EdgeType { Start, End };
struct BoundEdge { Float t; uint32_t primNum; EdgeType type; };
struct BuildNode { uint32_t depth, nPrimitives, badRefines; std::vector<Bnds> nodeBounds; KMesh mesh; Float area; uint32_t *primNums; uint32_t parentNum; };

// false: the reference's undefined case (only the fixed-cost minimum is finite, rbspKd.cpp:423-455)
bool Build(const std::vector<Prim> &prims, uint32_t M, uint32_t isectCost, uint32_t traversalCost, uint32_t kdTraversalCost, Float emptyBonus,
           uint32_t maxPrims, uint32_t maxDepth, Tree *tree) {
    const Float BSP_ALPHA = 0.1;
    const size_t N = prims.size();
    if (maxDepth == (uint32_t)-1) {
        const int lg = N ? 63 - __builtin_clzll((uint64_t)N) : -1;
        maxDepth = (uint32_t)std::round(2 + 1.6f * lg);
    }
    tree->M = M;
    tree->dirs = Directions(M);
    const std::vector<V3> &dirs = tree->dirs;
    const uint32_t off = BitOffset(M);
    std::vector<Bnds> rootB(M);
    std::vector<std::vector<Bnds>> all;
    tree->bounds = B3();
    for (const Prim &p : prims) {
        tree->bounds = Union(tree->bounds, p.wb);
        std::vector<Bnds> mb;
        for (uint32_t i = 0; i < M; ++i) {
            Bnds b;
            if (p.tri) {
                Float t = Dot(dirs[i], p.p[0]);
                Float mn = t, mx = t;
                for (int k = 1; k < 3; ++k) { t = Dot(dirs[i], p.p[k]); if (t > mx) mx = t; else if (t < mn) mn = t; }
                b.min = mn; b.max = mx;
            } else {
                for (int c = 0; c < 8; ++c) {
                    const V3 q((c & 1) ? p.wb.pMax.x : p.wb.pMin.x, (c & 2) ? p.wb.pMax.y : p.wb.pMin.y, (c & 4) ? p.wb.pMax.z : p.wb.pMin.z);
                    const float proj = Dot(dirs[i], q);
                    if (proj < b.min) b.min = proj;
                    if (proj > b.max) b.max = proj;
                }
            }
            mb.push_back(b);
            rootB[i] = Union(rootB[i], b);
        }
        all.push_back(mb);
    }
    KMesh root;
    {
        const B3 &b = tree->bounds;
        V3 v1 = b.pMin, v2(b.pMin.x, b.pMin.y, b.pMax.z), v3(b.pMin.x, b.pMax.y, b.pMin.z), v4(b.pMax.x, b.pMin.y, b.pMin.z);
        V3 v5(b.pMin.x, b.pMax.y, b.pMax.z), v6(b.pMax.x, b.pMin.y, b.pMax.z), v7(b.pMax.x, b.pMax.y, b.pMin.z), v8 = b.pMax;
        root.edges = {{v1, v2, 1, 3}, {v1, v3, 1, 5}, {v1, v4, 3, 5}, {v2, v5, 1, 4}, {v2, v6, 3, 4}, {v3, v5, 1, 2},
                      {v3, v7, 2, 5}, {v4, v6, 0, 3}, {v4, v7, 0, 5}, {v5, v8, 2, 4}, {v6, v8, 0, 4}, {v7, v8, 0, 2}};
    }
    std::vector<std::vector<BoundEdge>> edges(M, std::vector<BoundEdge>(2 * N));
    std::vector<uint32_t> primsBuf((size_t)(maxDepth + 1) * N + 1);
    for (uint32_t i = 0; i < N; ++i) primsBuf[i] = i;
    std::vector<Node> &nodes = tree->nodes;
    auto InitLeaf = [&](uint32_t nodeNum, uint32_t *primNums, uint32_t np) {
        nodes[nodeNum].flags = M;
        nodes[nodeNum].nPrims |= (np << off);
        if (np == 0) nodes[nodeNum].onePrimitive = 0;
        else if (np == 1) nodes[nodeNum].onePrimitive = primNums[0];
        else {
            nodes[nodeNum].primitiveIndicesOffset = (uint32_t)tree->primitiveIndices.size();
            for (uint32_t i = 0; i < np; ++i) tree->primitiveIndices.push_back(primNums[i]);
        }
    };
    uint32_t nodeNum = 0;
    std::vector<BuildNode> stack;
    const Float rootArea = MeshArea(root.edges, dirs);
    stack.push_back(BuildNode{maxDepth, (uint32_t)N, 0, rootB, root, rootArea, &primsBuf[0], (uint32_t)-1});
    while (!stack.empty()) {
        BuildNode cur = stack.back();
        stack.pop_back();
        if (cur.parentNum != (uint32_t)-1) nodes[cur.parentNum].aboveChild |= (nodeNum << off);
        nodes.emplace_back();
        if (cur.nPrimitives <= maxPrims || cur.depth == 0) { InitLeaf(nodeNum++, cur.primNums, cur.nPrimitives); continue; }
        uint32_t bestD = (uint32_t)-1, bestOffset = (uint32_t)-1, bestDFixed = (uint32_t)-1;
        std::pair<KMesh, KMesh> best;
        std::pair<Float, Float> bestAreas(0, 0);
        Float bestCost = Infinity, bestCostFixed = Infinity;
        const Float oldCost = isectCost * Float(cur.nPrimitives);
        const Float invTotalSA = 1 / cur.area;
        for (uint32_t d = 0; d < M; ++d) {     // d < 3: the kd sweep; d >= 3: the oblique sweep with its second minimum
            for (uint32_t i = 0; i < cur.nPrimitives; ++i) {
                const uint32_t pn = cur.primNums[i];
                edges[d][2 * i] = BoundEdge{all[pn][d].min, pn, EdgeType::Start};
                edges[d][2 * i + 1] = BoundEdge{all[pn][d].max, pn, EdgeType::End};
            }
            std::sort(&edges[d][0], &edges[d][0] + 2 * cur.nPrimitives, [](const BoundEdge &e0, const BoundEdge &e1) -> bool {
                if (e0.t == e1.t) return (int)e0.type < (int)e1.type;
                else return e0.t < e1.t;
            });
            uint32_t nBelow = 0, nAbove = cur.nPrimitives;
            for (uint32_t i = 0; i < 2 * cur.nPrimitives; ++i) {
                if (edges[d][i].type == EdgeType::End) --nAbove;
                const Float edgeT = edges[d][i].t;
                if (edgeT > cur.nodeBounds[d].min && edgeT < cur.nodeBounds[d].max) {
                    std::pair<KMesh, KMesh> cut = CutMesh(cur.mesh.edges, M, edgeT, dirs[d], d);
                    const Float areaBelow = MeshArea(cut.first.edges, dirs), areaAbove = MeshArea(cut.second.edges, dirs);
                    const Float pBelow = areaBelow * invTotalSA, pAbove = areaAbove * invTotalSA;
                    const Float eb = (nAbove == 0 || nBelow == 0) ? emptyBonus : 0;
                    if (d < 3) {
                        const Float cost = kdTraversalCost + isectCost * (1 - eb) * (pBelow * nBelow + pAbove * nAbove);
                        if (cost < bestCost) { bestCost = cost; bestD = d; bestOffset = i; best = cut; bestAreas = std::make_pair(areaBelow, areaAbove); }
                    } else {
                        const Float costIntersection = isectCost * (1 - eb) * (pBelow * nBelow + pAbove * nAbove);
                        const Float costFixed = traversalCost + costIntersection;
                        const Float cost = BSP_ALPHA * isectCost * (cur.nPrimitives - 1) + kdTraversalCost + costIntersection;
                        if (cost < bestCost) { bestCost = cost; bestD = d; bestOffset = i; best = cut; bestAreas = std::make_pair(areaBelow, areaAbove); }
                        if (costFixed < bestCostFixed) { bestCostFixed = costFixed; bestDFixed = d; }
                    }
                }
                if (edges[d][i].type == EdgeType::Start) ++nBelow;
            }
        }
        if (bestCost > oldCost && bestCostFixed > oldCost) ++cur.badRefines;
        if ((bestCost > 4 * oldCost && bestCostFixed > 4 * oldCost && cur.nPrimitives < 16) || (bestD == (uint32_t)-1 && bestDFixed == (uint32_t)-1) ||
            cur.badRefines == 3) {
            InitLeaf(nodeNum++, cur.primNums, cur.nPrimitives);
            continue;
        }
        if (bestD == (uint32_t)-1) return false;
        uint32_t n0 = 0, n1 = 0;
        uint32_t *prims1 = cur.primNums;
        for (uint32_t i = bestOffset + 1; i < 2 * cur.nPrimitives; ++i)
            if (edges[bestD][i].type == EdgeType::End) prims1[n1++] = edges[bestD][i].primNum;
        uint32_t *prims0 = prims1 + n1;
        for (uint32_t i = 0; i < bestOffset; ++i)
            if (edges[bestD][i].type == EdgeType::Start) prims0[n0++] = edges[bestD][i].primNum;
        const Float tSplit = edges[bestD][bestOffset].t;
        std::vector<Bnds> b0(M), b1(M);
        for (uint32_t d = 0; d < M; ++d) {
            for (auto &e : best.first.edges) b0[d] = Union(b0[d], e.getBounds(dirs[d]));
            for (auto &e : best.second.edges) b1[d] = Union(b1[d], e.getBounds(dirs[d]));
        }
        nodes[nodeNum].split = tSplit;
        nodes[nodeNum].flags = bestD;
        stack.push_back(BuildNode{cur.depth - 1, n1, cur.badRefines, b1, best.second, bestAreas.second, prims1, nodeNum});
        stack.push_back(BuildNode{cur.depth - 1, n0, cur.badRefines, b0, best.first, bestAreas.first, prims0, (uint32_t)-1});
        ++nodeNum;
    }
    return true;
}

// Bounds3::IntersectP(const Ray &, Float *, Float *), core/geometry.h:1730-1751
bool RootInterval(const B3 &b, const Ray &ray, Float *hitt0, Float *hitt1) {
    Float t0 = 0, t1 = ray.tMax;
    for (int i = 0; i < 3; ++i) {
        Float invRayDir = 1 / ray.d[i];
        Float tNear = (b.pMin[i] - ray.o[i]) * invRayDir;
        Float tFar = (b.pMax[i] - ray.o[i]) * invRayDir;
        if (tNear > tFar) std::swap(tNear, tFar);
        tFar *= 1 + 2 * gamma(3);
        t0 = tNear > t0 ? tNear : t0;
        t1 = tFar < t1 ? tFar : t1;
        if (t0 > t1) return false;
    }
    *hitt0 = t0; *hitt1 = t1;
    return true;
}

struct WalkCount { uint64_t nodes = 0, interior = 0, leaves = 0, kd = 0; };     // interior: kd + bsp
struct ToDo { const Node *node; Float tMin, tMax; };

struct SceneRef {
    Scene scene;
    std::vector<BVH> objectBvh;
    BVH bvh;                       // primOrder: ordered -> creation number (the device numbering), and the primitive tests
    std::vector<uint32_t> toOrdered;
    Tree tree;

    bool dotOnly = false;          // the control: RBSP's dot-product step at every node, axis nodes included

    // RBSPKdNode::intersectInterior (rbspKd.cpp:69-92): planeDistance(split, ray, invDir, axis) at axis nodes, the direction's
    // planeDistance (core/geometry.h:1833-1843) at oblique ones
    void Interior(const Node *node, const Ray &ray, const V3 &invDir, Float *tPlane, bool *belowFirst) const {
        const uint32_t axis = node->flags & BitMask(tree.M);
        if (axis < 3 && !dotOnly) {
            *tPlane = (node->split - ray.o[axis]) * invDir[axis];
            *belowFirst = (ray.o[axis] < node->split) || (ray.o[axis] == node->split && ray.d[axis] <= 0);
            return;
        }
        const V3 &dir = tree.dirs[axis];
        const Float projectedO = Dot(dir, ray.o);
        const Float inverseProjectedD = 1 / Dot(dir, ray.d);
        *tPlane = (node->split - projectedO) * inverseProjectedD;
        *belowFirst = (projectedO < node->split) || (projectedO == node->split && inverseProjectedD <= 0);
    }
    bool IsLeaf(const Node *n) const { return (n->flags & BitMask(tree.M)) == tree.M; }

    // RBSPKd::Intersect, accelerators/rbspKd.cpp:490-565
    bool Intersect(const Ray &ray, SurfaceInteraction *isect, Counters &ctr, WalkCount &wc) const {
        const uint32_t off = BitOffset(tree.M);
        Float tMin, tMax;
        if (!RootInterval(tree.bounds, ray, &tMin, &tMax)) return false;
        const V3 invDir(1 / ray.d.x, 1 / ray.d.y, 1 / ray.d.z);
        ToDo todo[64];
        uint32_t todoPos = 0;
        bool hit = false;
        const Node *node = &tree.nodes[0];
        while (node != nullptr) {
            if (ray.tMax < tMin) break;
            ++wc.nodes;
            if (!IsLeaf(node)) {
                ++wc.interior;
                if ((node->flags & BitMask(tree.M)) < 3) ++wc.kd;
                Float tPlane; bool belowFirst;
                Interior(node, ray, invDir, &tPlane, &belowFirst);
                const Node *first, *second;
                if (belowFirst) { first = node + 1; second = &tree.nodes[node->aboveChild >> off]; }
                else { first = &tree.nodes[node->aboveChild >> off]; second = node + 1; }
                if (tPlane > tMax || tPlane <= 0) node = first;
                else if (tPlane < tMin) node = second;
                else { todo[todoPos].node = second; todo[todoPos].tMin = tPlane; todo[todoPos].tMax = tMax; ++todoPos; node = first; tMax = tPlane; }
            } else {
                ++wc.leaves;
                const uint32_t np = node->nPrims >> off;
                for (uint32_t i = 0; i < np; ++i) {
                    const uint32_t p = np == 1 ? node->onePrimitive : tree.primitiveIndices[node->primitiveIndicesOffset + i];
                    if (bvh.PrimIntersect(toOrdered[p], ray, isect, ctr)) hit = true;
                }
                if (todoPos > 0) { --todoPos; node = todo[todoPos].node; tMin = todo[todoPos].tMin; tMax = todo[todoPos].tMax; }
                else break;
            }
        }
        return hit;
    }
    // RBSPKd::IntersectP, :567-638
    bool IntersectP(const Ray &ray, Counters &ctr, WalkCount &wc) const {
        const uint32_t off = BitOffset(tree.M);
        Float tMin, tMax;
        if (!RootInterval(tree.bounds, ray, &tMin, &tMax)) return false;
        const V3 invDir(1 / ray.d.x, 1 / ray.d.y, 1 / ray.d.z);
        ToDo todo[64];
        uint32_t todoPos = 0;
        const Node *node = &tree.nodes[0];
        while (node != nullptr) {
            ++wc.nodes;
            if (IsLeaf(node)) {
                ++wc.leaves;
                const uint32_t np = node->nPrims >> off;
                for (uint32_t i = 0; i < np; ++i) {
                    const uint32_t p = np == 1 ? node->onePrimitive : tree.primitiveIndices[node->primitiveIndicesOffset + i];
                    if (bvh.PrimIntersectP(toOrdered[p], ray, ctr)) return true;
                }
                if (todoPos > 0) { --todoPos; node = todo[todoPos].node; tMin = todo[todoPos].tMin; tMax = todo[todoPos].tMax; }
                else break;
            } else {
                ++wc.interior;
                if ((node->flags & BitMask(tree.M)) < 3) ++wc.kd;
                Float tPlane; bool belowFirst;
                Interior(node, ray, invDir, &tPlane, &belowFirst);
                const Node *first, *second;
                if (belowFirst) { first = node + 1; second = &tree.nodes[node->aboveChild >> off]; }
                else { first = &tree.nodes[node->aboveChild >> off]; second = node + 1; }
                if (tPlane > tMax || tPlane <= 0) node = first;
                else if (tPlane < tMin) node = second;
                else { todo[todoPos].node = second; todo[todoPos].tMin = tPlane; todo[todoPos].tMax = tMax; ++todoPos; node = first; tMax = tPlane; }
            }
        }
        return false;
    }

    std::vector<Prim> Prims() const {
        std::vector<Prim> out(scene.prims.size());
        for (size_t i = 0; i < out.size(); ++i) {
            const PrimRef &pr = scene.prims[i];
            out[i].wb = bvh.PrimWorldBound((uint32_t)i);
            const ShapeRec &sh = scene.shapes[pr.shape];
            out[i].tri = sh.kind == SHAPE_MESH;
            if (out[i].tri) {
                const Mesh &m = scene.meshes[sh.meshIndex];
                for (int k = 0; k < 3; ++k) out[i].p[k] = m.p[m.idx[3 * pr.local + k]];
            }
        }
        return out;
    }
};

std::string g_err;

void CopyTree(const Tree &t, void *nodes8, uint32_t *idx, float *dirs) {
    if (nodes8) memcpy(nodes8, t.nodes.data(), t.nodes.size() * 8);
    if (idx && !t.primitiveIndices.empty()) memcpy(idx, t.primitiveIndices.data(), t.primitiveIndices.size() * 4);
    if (dirs) for (size_t k = 0; k < t.dirs.size(); ++k) { dirs[3 * k] = t.dirs[k].x; dirs[3 * k + 1] = t.dirs[k].y; dirs[3 * k + 2] = t.dirs[k].z; }
}

}  // namespace

extern "C" {

const char *rbspkdref_last_error() { return g_err.c_str(); }

// build over n triangles (9 floats each, creation order); sizes[0..1] = nodes, primitiveIndices entries
// returns null (rbspkdref_last_error) where the reference's build is undefined
void *rbspkdref_build(size_t n, const float *p9, int M, int isectCost, int travCost, int kdTravCost, float emptyBonus, int maxPrims, int maxDepth,
                      uint32_t sizes[2]) {
    std::vector<Prim> prims(n);
    for (size_t i = 0; i < n; ++i) {
        Prim &p = prims[i];
        p.tri = true;
        for (int k = 0; k < 3; ++k) p.p[k] = V3(p9[9 * i + 3 * k], p9[9 * i + 3 * k + 1], p9[9 * i + 3 * k + 2]);
        p.wb = Union(B3(p.p[0], p.p[1]), p.p[2]);
    }
    Tree *t = new Tree();
    if (!Build(prims, (uint32_t)M, (uint32_t)isectCost, (uint32_t)travCost, (uint32_t)kdTravCost, emptyBonus, (uint32_t)maxPrims, (uint32_t)maxDepth, t)) {
        g_err = "only the fixed-cost minimum is finite"; delete t; return nullptr;
    }
    sizes[0] = (uint32_t)t->nodes.size(); sizes[1] = (uint32_t)t->primitiveIndices.size();
    return t;
}
void rbspkdref_copy(void *h, void *nodes8, uint32_t *idx, float *dirs) { CopyTree(*(const Tree *)h, nodes8, idx, dirs); }
void rbspkdref_free(void *h) { delete (Tree *)h; }

// a baked scene (no instances) and its BVH (for the ordered numbering).  build != 0: the restated tree over its primitives
// with nbDirections M and the other defaults; else the tree is given with rbspkdref_scene_set_tree.
void *rbspkdref_scene_load(const char *path, int M, int build) {
    SceneRef *r = new SceneRef();
    std::string err;
    if (!LoadScene(path, &r->scene, &err)) { g_err = err; delete r; return nullptr; }
    if (!r->scene.instances.empty()) { g_err = "instanced scene"; delete r; return nullptr; }
    r->bvh.Build(&r->scene, &r->scene.prims, &r->objectBvh, 0);
    const size_t n = r->scene.prims.size();
    r->toOrdered.resize(n);
    for (size_t i = 0; i < n; ++i) r->toOrdered[r->bvh.primOrder[i]] = (uint32_t)i;
    r->tree.M = (uint32_t)M;
    r->tree.dirs = Directions((uint32_t)M);
    r->tree.bounds = B3();
    for (size_t i = 0; i < n; ++i) r->tree.bounds = Union(r->tree.bounds, r->bvh.PrimWorldBound((uint32_t)i));
    if (build && !Build(r->Prims(), (uint32_t)M, 80, 5, 1, 0.f, 1, (uint32_t)-1, &r->tree)) { g_err = "only the fixed-cost minimum is finite"; delete r; return nullptr; }
    return r;
}
void rbspkdref_scene_set_tree(void *h, int M, size_t nNodes, const void *nodes8, size_t nIdx, const uint32_t *idx) {
    SceneRef *r = (SceneRef *)h;
    r->tree.M = (uint32_t)M;
    r->tree.dirs = Directions((uint32_t)M);
    r->tree.nodes.resize(nNodes);
    memcpy(r->tree.nodes.data(), nodes8, nNodes * 8);
    r->tree.primitiveIndices.assign(idx, idx + nIdx);
}
void rbspkdref_scene_free(void *h) { delete (SceneRef *)h; }
size_t rbspkdref_scene_prims(void *h) { return ((SceneRef *)h)->scene.prims.size(); }
// the scene's triangles in creation order (9 floats each; other primitives are skipped); returns how many
size_t rbspkdref_scene_triangles(void *h, float *p9) {
    size_t k = 0;
    for (const Prim &p : ((SceneRef *)h)->Prims())
        if (p.tri) { for (int v = 0; v < 3; ++v) { p9[9 * k + 3 * v] = p.p[v].x; p9[9 * k + 3 * v + 1] = p.p[v].y; p9[9 * k + 3 * v + 2] = p.p[v].z; } ++k; }
    return k;
}
void rbspkdref_scene_tree(void *h, uint32_t sizes[2], void *nodes8, uint32_t *idx) {
    SceneRef *r = (SceneRef *)h;
    sizes[0] = (uint32_t)r->tree.nodes.size(); sizes[1] = (uint32_t)r->tree.primitiveIndices.size();
    if (nodes8) CopyTree(r->tree, nodes8, idx, nullptr);
}
// the split planes of the scene's tree (direction, position) of the first `cap` interior nodes
size_t rbspkdref_scene_splits(void *h, int32_t *axis, float *pos, size_t cap) {
    SceneRef *r = (SceneRef *)h;
    size_t k = 0;
    for (const Node &nd : r->tree.nodes)
        if ((nd.flags & BitMask(r->tree.M)) != r->tree.M && k < cap) { axis[k] = (int32_t)(nd.flags & BitMask(r->tree.M)); pos[k] = nd.split; ++k; }
    return k;
}
// dot != 0: walk every interior node with the dot-product step (the control)
void rbspkdref_scene_dot_only(void *h, int dot) { ((SceneRef *)h)->dotOnly = dot != 0; }
// counters5 per ray: nodes (nbNodeTraversals), interior (kd + bsp), triangle tests, sphere tests, kd interior nodes
void rbspkdref_intersect(void *h, size_t n, const float *o, const float *d, const float *tmax, float *tOut, int32_t *primOut, float *bary,
                       uint64_t *counters5) {
    SceneRef *r = (SceneRef *)h;
    for (size_t i = 0; i < n; ++i) {
        Ray ray(V3(o[3 * i], o[3 * i + 1], o[3 * i + 2]), V3(d[3 * i], d[3 * i + 1], d[3 * i + 2]), tmax[i]);
        SurfaceInteraction si; Counters c; WalkCount wc;
        const bool hit = r->Intersect(ray, &si, c, wc);
        tOut[i] = ray.tMax; primOut[i] = hit ? si.ordered : -1;
        bary[3 * i] = hit ? si.b0 : 0.f; bary[3 * i + 1] = hit ? si.b1 : 0.f; bary[3 * i + 2] = hit ? si.b2 : 0.f;
        counters5[5 * i] = wc.nodes; counters5[5 * i + 1] = wc.interior; counters5[5 * i + 2] = c.triTests; counters5[5 * i + 3] = c.sphereTests;
        counters5[5 * i + 4] = wc.kd;
    }
}
void rbspkdref_occluded(void *h, size_t n, const float *o, const float *d, const float *tmax, uint8_t *occ, uint64_t *counters5) {
    SceneRef *r = (SceneRef *)h;
    for (size_t i = 0; i < n; ++i) {
        Ray ray(V3(o[3 * i], o[3 * i + 1], o[3 * i + 2]), V3(d[3 * i], d[3 * i + 1], d[3 * i + 2]), tmax[i]);
        Counters c; WalkCount wc;
        occ[i] = r->IntersectP(ray, c, wc) ? 1 : 0;
        counters5[5 * i] = wc.nodes; counters5[5 * i + 1] = wc.interior; counters5[5 * i + 2] = c.triTestsP; counters5[5 * i + 3] = c.sphereTestsP;
        counters5[5 * i + 4] = wc.kd;
    }
}

}  // extern "C"
