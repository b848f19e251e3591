// Test-side restatement of the fork's kd-tree (accelerators/kdtreeaccel.cpp:212-521): KdTreeAccel::buildTree and the two
// walks, Intersect and IntersectP, written independently of thesis-pbrt-v3_amd/csrc/ over the oracle's primitive tests
// (oracle/orc_accel.h, included read-only).  Compiled with g++ at test time (tests/kd_ref.py) and driven through ctypes.
// It pins nothing against a reference binary: the device walk is held to THIS walk ("parity unpinned").
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>
#include "orc_accel.h"

namespace orc { bool g_use_libm = false; }
using namespace orc;

namespace {

struct Node {                       // KdAccelNode: union { split, onePrimitive, primitiveIndicesOffset }; union { flags, nPrims, aboveChild }
    union { float split; uint32_t onePrimitive; uint32_t primitiveIndicesOffset; };
    union { uint32_t flags; uint32_t nPrims; uint32_t aboveChild; };
};
static_assert(sizeof(Node) == 8, "KdAccelNode is 8 bytes");

struct Tree {
    std::vector<Node> nodes;
    std::vector<uint32_t> primitiveIndices;
    B3 bounds;
};

enum class EdgeType { Start, End };
struct BoundEdge { Float t; uint32_t primNum; EdgeType type; };
struct BuildNode { uint32_t depth, nPrimitives, badRefines; B3 nodeBounds; uint32_t *primNums; uint32_t parentNum; };

void Build(const std::vector<B3> &allPrimBounds, uint32_t isectCost, uint32_t traversalCost, Float emptyBonus, uint32_t maxPrims,
           uint32_t maxDepth, Tree *tree) {
    const size_t N = allPrimBounds.size();
    if (maxDepth == (uint32_t)-1) {
        const int lg = N ? 63 - __builtin_clzll((uint64_t)N) : -1;
        maxDepth = (uint32_t)std::round(2 + 1.6f * lg);
    }
    tree->bounds = B3();
    for (const B3 &b : allPrimBounds) tree->bounds = Union(tree->bounds, b);
    std::vector<BoundEdge> edges[3];
    for (auto &e : edges) e.resize(2 * N);
    std::vector<uint32_t> prims((size_t)(maxDepth + 1) * N + 1);
    for (uint32_t i = 0; i < N; ++i) prims[i] = i;
    std::vector<Node> &nodes = tree->nodes;
    auto InitLeaf = [&](uint32_t nodeNum, uint32_t *primNums, uint32_t np) {
        nodes[nodeNum].flags = 3u;
        nodes[nodeNum].nPrims |= (np << 2u);
        if (np == 0) nodes[nodeNum].onePrimitive = 0;
        else if (np == 1) nodes[nodeNum].onePrimitive = primNums[0];
        else {
            nodes[nodeNum].primitiveIndicesOffset = (uint32_t)tree->primitiveIndices.size();
            for (uint32_t i = 0; i < np; ++i) tree->primitiveIndices.push_back(primNums[i]);
        }
    };
    uint32_t nodeNum = 0;
    std::vector<BuildNode> stack;
    stack.push_back(BuildNode{maxDepth, (uint32_t)N, 0, tree->bounds, &prims[0], (uint32_t)-1});
    while (!stack.empty()) {
        BuildNode cur = stack.back();
        stack.pop_back();
        if (cur.parentNum != (uint32_t)-1) nodes[cur.parentNum].aboveChild |= (nodeNum << 2u);
        nodes.emplace_back();
        if (cur.nPrimitives <= maxPrims || cur.depth == 0) { InitLeaf(nodeNum++, cur.primNums, cur.nPrimitives); continue; }
        uint32_t bestAxis = (uint32_t)-1, bestOffset = (uint32_t)-1;
        Float bestCost = Infinity;
        const Float oldCost = isectCost * Float(cur.nPrimitives);
        const Float totalSA = cur.nodeBounds.SurfaceArea();
        const Float invTotalSA = 1 / totalSA;
        const V3 d = cur.nodeBounds.pMax - cur.nodeBounds.pMin;
        for (uint32_t axis = 0; axis < 3; ++axis) {
            for (uint32_t i = 0; i < cur.nPrimitives; ++i) {
                const uint32_t pn = cur.primNums[i];
                const B3 &b = allPrimBounds[pn];
                edges[axis][2 * i] = BoundEdge{b.pMin[axis], pn, EdgeType::Start};
                edges[axis][2 * i + 1] = BoundEdge{b.pMax[axis], pn, EdgeType::End};
            }
            std::sort(&edges[axis][0], &edges[axis][0] + 2 * cur.nPrimitives, [](const BoundEdge &e0, const BoundEdge &e1) -> bool {
                if (e0.t == e1.t) return (int)e0.type < (int)e1.type;
                else return e0.t < e1.t;
            });
            uint32_t nBelow = 0, nAbove = cur.nPrimitives;
            for (uint32_t i = 0; i < 2 * cur.nPrimitives; ++i) {
                if (edges[axis][i].type == EdgeType::End) --nAbove;
                const Float edgeT = edges[axis][i].t;
                if (edgeT > cur.nodeBounds.pMin[axis] && edgeT < cur.nodeBounds.pMax[axis]) {
                    const uint32_t o0 = (axis + 1) % 3, o1 = (axis + 2) % 3;
                    const Float belowSA = 2 * (d[o0] * d[o1] + (edgeT - cur.nodeBounds.pMin[axis]) * (d[o0] + d[o1]));
                    const Float aboveSA = 2 * (d[o0] * d[o1] + (cur.nodeBounds.pMax[axis] - edgeT) * (d[o0] + d[o1]));
                    const Float pBelow = belowSA * invTotalSA, pAbove = aboveSA * invTotalSA;
                    const Float eb = (nAbove == 0 || nBelow == 0) ? emptyBonus : 0;
                    const Float cost = traversalCost + isectCost * (1 - eb) * (pBelow * nBelow + pAbove * nAbove);
                    if (cost < bestCost) { bestCost = cost; bestAxis = axis; bestOffset = i; }
                }
                if (edges[axis][i].type == EdgeType::Start) ++nBelow;
            }
        }
        if (bestCost > oldCost) ++cur.badRefines;
        if ((bestCost > 4 * oldCost && cur.nPrimitives < 16) || bestAxis == (uint32_t)-1 || cur.badRefines == 3) {
            InitLeaf(nodeNum++, cur.primNums, cur.nPrimitives);
            continue;
        }
        uint32_t n0 = 0, n1 = 0;
        uint32_t *prims1 = cur.primNums;
        for (uint32_t i = bestOffset + 1; i < 2 * cur.nPrimitives; ++i)
            if (edges[bestAxis][i].type == EdgeType::End) prims1[n1++] = edges[bestAxis][i].primNum;
        uint32_t *prims0 = prims1 + n1;
        for (uint32_t i = 0; i < bestOffset; ++i)
            if (edges[bestAxis][i].type == EdgeType::Start) prims0[n0++] = edges[bestAxis][i].primNum;
        const Float tSplit = edges[bestAxis][bestOffset].t;
        B3 bounds0 = cur.nodeBounds, bounds1 = cur.nodeBounds;
        bounds0.pMax[bestAxis] = bounds1.pMin[bestAxis] = tSplit;
        nodes[nodeNum].split = tSplit;
        nodes[nodeNum].flags = bestAxis;
        stack.push_back(BuildNode{cur.depth - 1, n1, cur.badRefines, bounds1, prims1, nodeNum});
        stack.push_back(BuildNode{cur.depth - 1, n0, cur.badRefines, bounds0, prims0, (uint32_t)-1});
        ++nodeNum;
    }
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

struct WalkCount { uint64_t nodes = 0, interior = 0, leaves = 0; };
struct ToDo { const Node *node; Float tMin, tMax; };

struct SceneRef {
    Scene scene;
    std::vector<BVH> objectBvh;
    BVH bvh;                       // primOrder: ordered -> creation number (the device numbering), and the primitive tests
    std::vector<uint32_t> toOrdered;
    Tree tree;

    // KdTreeAccel::Intersect, accelerators/kdtreeaccel.cpp:381-457
    bool Intersect(const Ray &ray, SurfaceInteraction *isect, Counters &ctr, WalkCount &wc) const {
        Float tMin, tMax;
        if (!RootInterval(tree.bounds, ray, &tMin, &tMax)) return false;
        V3 invDir(1 / ray.d.x, 1 / ray.d.y, 1 / ray.d.z);
        ToDo todo[64];
        uint32_t todoPos = 0;
        bool hit = false;
        const Node *node = &tree.nodes[0];
        while (node != nullptr) {
            if (ray.tMax < tMin) break;
            ++wc.nodes;
            if ((node->flags & 3u) != 3u) {
                ++wc.interior;
                const uint32_t axis = node->flags & 3u;
                const Float tPlane = (node->split - ray.o[axis]) * invDir[axis];
                const bool belowFirst = (ray.o[axis] < node->split) || (ray.o[axis] == node->split && ray.d[axis] <= 0);
                const Node *first, *second;
                if (belowFirst) { first = node + 1; second = &tree.nodes[node->aboveChild >> 2]; }
                else { first = &tree.nodes[node->aboveChild >> 2]; second = node + 1; }
                if (tPlane > tMax || tPlane <= 0) node = first;
                else if (tPlane < tMin) node = second;
                else { todo[todoPos].node = second; todo[todoPos].tMin = tPlane; todo[todoPos].tMax = tMax; ++todoPos; node = first; tMax = tPlane; }
            } else {
                ++wc.leaves;
                const uint32_t np = node->nPrims >> 2;
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
    // KdTreeAccel::IntersectP, :459-521
    bool IntersectP(const Ray &ray, Counters &ctr, WalkCount &wc) const {
        Float tMin, tMax;
        if (!RootInterval(tree.bounds, ray, &tMin, &tMax)) return false;
        V3 invDir(1 / ray.d.x, 1 / ray.d.y, 1 / ray.d.z);
        ToDo todo[64];
        uint32_t todoPos = 0;
        const Node *node = &tree.nodes[0];
        while (node != nullptr) {
            ++wc.nodes;
            if ((node->flags & 3u) == 3u) {
                ++wc.leaves;
                const uint32_t np = node->nPrims >> 2;
                for (uint32_t i = 0; i < np; ++i) {
                    const uint32_t p = np == 1 ? node->onePrimitive : tree.primitiveIndices[node->primitiveIndicesOffset + i];
                    if (bvh.PrimIntersectP(toOrdered[p], ray, ctr)) return true;
                }
                if (todoPos > 0) { --todoPos; node = todo[todoPos].node; tMin = todo[todoPos].tMin; tMax = todo[todoPos].tMax; }
                else break;
            } else {
                ++wc.interior;
                const uint32_t axis = node->flags & 3u;
                const Float tPlane = (node->split - ray.o[axis]) * invDir[axis];
                const bool belowFirst = (ray.o[axis] < node->split) || (ray.o[axis] == node->split && ray.d[axis] <= 0);
                const Node *first, *second;
                if (belowFirst) { first = node + 1; second = &tree.nodes[node->aboveChild >> 2]; }
                else { first = &tree.nodes[node->aboveChild >> 2]; second = node + 1; }
                if (tPlane > tMax || tPlane <= 0) node = first;
                else if (tPlane < tMin) node = second;
                else { todo[todoPos].node = second; todo[todoPos].tMin = tPlane; todo[todoPos].tMax = tMax; ++todoPos; node = first; tMax = tPlane; }
            }
        }
        return false;
    }
};

std::string g_err;

}  // namespace

extern "C" {

const char *kdref_last_error() { return g_err.c_str(); }

// build from creation-order bounds; sizes[0..1] = nodes, primitiveIndices entries
void *kdref_build(size_t n, const float *bmin, const float *bmax, int isectCost, int travCost, float emptyBonus, int maxPrims, int maxDepth,
                  uint32_t sizes[2]) {
    std::vector<B3> b(n);
    for (size_t i = 0; i < n; ++i) {
        b[i].pMin = V3(bmin[3 * i], bmin[3 * i + 1], bmin[3 * i + 2]);
        b[i].pMax = V3(bmax[3 * i], bmax[3 * i + 1], bmax[3 * i + 2]);
    }
    Tree *t = new Tree();
    Build(b, (uint32_t)isectCost, (uint32_t)travCost, emptyBonus, (uint32_t)maxPrims, (uint32_t)maxDepth, t);
    sizes[0] = (uint32_t)t->nodes.size(); sizes[1] = (uint32_t)t->primitiveIndices.size();
    return t;
}
void kdref_copy(void *h, void *nodes8, uint32_t *idx) {
    const Tree *t = (const Tree *)h;
    memcpy(nodes8, t->nodes.data(), t->nodes.size() * 8);
    if (!t->primitiveIndices.empty()) memcpy(idx, t->primitiveIndices.data(), t->primitiveIndices.size() * 4);
}
void kdref_free(void *h) { delete (Tree *)h; }

// a baked scene (no instances), its BVH (for the ordered numbering) and the default kd-tree over its primitives
void *kdref_scene_load(const char *path) {
    SceneRef *r = new SceneRef();
    std::string err;
    if (!LoadScene(path, &r->scene, &err)) { g_err = err; delete r; return nullptr; }
    if (!r->scene.instances.empty()) { g_err = "instanced scene"; delete r; return nullptr; }
    r->bvh.Build(&r->scene, &r->scene.prims, &r->objectBvh, 0);
    const size_t n = r->scene.prims.size();
    r->toOrdered.resize(n);
    for (size_t i = 0; i < n; ++i) r->toOrdered[r->bvh.primOrder[i]] = (uint32_t)i;
    std::vector<B3> b(n);
    for (size_t i = 0; i < n; ++i) b[i] = r->bvh.PrimWorldBound((uint32_t)i);
    Build(b, 80, 1, 0.f, 1, (uint32_t)-1, &r->tree);
    return r;
}
void kdref_scene_free(void *h) { delete (SceneRef *)h; }
size_t kdref_scene_prims(void *h) { return ((SceneRef *)h)->scene.prims.size(); }
void kdref_scene_bounds(void *h, float *bmin, float *bmax) {
    SceneRef *r = (SceneRef *)h;
    for (size_t i = 0; i < r->scene.prims.size(); ++i) {
        const B3 b = r->bvh.PrimWorldBound((uint32_t)i);
        for (int k = 0; k < 3; ++k) { bmin[3 * i + k] = b.pMin[k]; bmax[3 * i + k] = b.pMax[k]; }
    }
}
void kdref_scene_tree(void *h, uint32_t sizes[2], void *nodes8, uint32_t *idx) {
    SceneRef *r = (SceneRef *)h;
    sizes[0] = (uint32_t)r->tree.nodes.size(); sizes[1] = (uint32_t)r->tree.primitiveIndices.size();
    if (nodes8) kdref_copy(&r->tree, nodes8, idx);
}
// the split planes of the scene's tree (axis, position) of the first `cap` interior nodes: rays with o[axis] == split
size_t kdref_scene_splits(void *h, int32_t *axis, float *pos, size_t cap) {
    SceneRef *r = (SceneRef *)h;
    size_t k = 0;
    for (const Node &nd : r->tree.nodes) if ((nd.flags & 3u) != 3u && k < cap) { axis[k] = (int32_t)(nd.flags & 3u); pos[k] = nd.split; ++k; }
    return k;
}
// counters4 per ray: nodes (nbNodeTraversals), interior (kdTreeNodeTraversals), triangle tests, sphere tests
void kdref_intersect(void *h, size_t n, const float *o, const float *d, const float *tmax, float *tOut, int32_t *primOut, float *bary,
                     uint64_t *counters4) {
    SceneRef *r = (SceneRef *)h;
    for (size_t i = 0; i < n; ++i) {
        Ray ray(V3(o[3 * i], o[3 * i + 1], o[3 * i + 2]), V3(d[3 * i], d[3 * i + 1], d[3 * i + 2]), tmax[i]);
        SurfaceInteraction si; Counters c; WalkCount wc;
        const bool hit = r->Intersect(ray, &si, c, wc);
        tOut[i] = ray.tMax; primOut[i] = hit ? si.ordered : -1;
        bary[3 * i] = hit ? si.b0 : 0.f; bary[3 * i + 1] = hit ? si.b1 : 0.f; bary[3 * i + 2] = hit ? si.b2 : 0.f;
        counters4[4 * i] = wc.nodes; counters4[4 * i + 1] = wc.interior; counters4[4 * i + 2] = c.triTests; counters4[4 * i + 3] = c.sphereTests;
    }
}
void kdref_occluded(void *h, size_t n, const float *o, const float *d, const float *tmax, uint8_t *occ, uint64_t *counters4) {
    SceneRef *r = (SceneRef *)h;
    for (size_t i = 0; i < n; ++i) {
        Ray ray(V3(o[3 * i], o[3 * i + 1], o[3 * i + 2]), V3(d[3 * i], d[3 * i + 1], d[3 * i + 2]), tmax[i]);
        Counters c; WalkCount wc;
        occ[i] = r->IntersectP(ray, c, wc) ? 1 : 0;
        counters4[4 * i] = wc.nodes; counters4[4 * i + 1] = wc.interior; counters4[4 * i + 2] = c.triTestsP; counters4[4 * i + 3] = c.sphereTestsP;
    }
}

}  // extern "C"
