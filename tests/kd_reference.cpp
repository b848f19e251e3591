// Test-side restatement of the fork's kd-tree (accelerators/kdtreeaccel.cpp:212-521): KdTreeAccel::buildTree and the interior
// step of the two walks, Intersect and IntersectP, which tests/tree_reference.h holds for the four tree accelerators, written
// independently of thesis-pbrt-v3_amd/csrc/ over the oracle's primitive tests (oracle/orc_accel.h, included read-only).
// Compiled with g++ at test time (tests/tree_ref.py) and driven through ctypes.
// It pins nothing against a reference binary: the device walk is held to THIS walk ("parity unpinned").
#include "tree_reference.h"

namespace {

typedef TreeT<Node> Tree;

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

// KdAccelNode: the axis in the two low bits, 3 a leaf; the interior step of kdtreeaccel.cpp:403-417
struct KdStep {
    typedef Node NodeT;
    static uint32_t Shift(const Tree &) { return 2; }
    static uint32_t Axis(const Tree &, const Node *n) { return n->flags & 3u; }
    static bool IsLeaf(const Tree &, const Node *n) { return (n->flags & 3u) == 3u; }
    static bool Kd(const Tree &, const Node *) { return false; }       // (only rbspkd counts its axis nodes apart)
    static void Interior(const Tree &, const Node *node, const Ray &ray, const V3 &invDir, Float *tPlane, bool *belowFirst) {
        const uint32_t axis = node->flags & 3u;
        *tPlane = (node->split - ray.o[axis]) * invDir[axis];
        *belowFirst = (ray.o[axis] < node->split) || (ray.o[axis] == node->split && ray.d[axis] <= 0);
    }
};
typedef SceneRef<KdStep> KdScene;

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
void kdref_copy(void *h, void *nodes8, uint32_t *idx) { CopyTree(*(const Tree *)h, nodes8, idx, nullptr); }
void kdref_free(void *h) { delete (Tree *)h; }

// a baked scene (no instances), its BVH (for the ordered numbering) and the default kd-tree over its primitives
void *kdref_scene_load(const char *path) {
    KdScene *r = LoadSceneRef<KdStep>(path);
    if (!r) return nullptr;
    const size_t n = r->scene.prims.size();
    std::vector<B3> b(n);
    for (size_t i = 0; i < n; ++i) b[i] = r->bvh.PrimWorldBound((uint32_t)i);
    Build(b, 80, 1, 0.f, 1, (uint32_t)-1, &r->tree);
    return r;
}
// the tree is given instead (a tree made by hand, or the library's)
void kdref_scene_set_tree(void *h, size_t nNodes, const void *nodes8, size_t nIdx, const uint32_t *idx) { SceneSetTree((KdScene *)h, nNodes, nodes8, nIdx, idx); }
size_t kdref_scene_max_todo(void *h, uint32_t *out) { return SceneMaxTodo((const KdScene *)h, out); }
void kdref_scene_free(void *h) { delete (KdScene *)h; }
size_t kdref_scene_prims(void *h) { return ((KdScene *)h)->scene.prims.size(); }
size_t kdref_scene_triangles(void *h, float *p9) { return SceneTriangles((const KdScene *)h, p9); }
void kdref_scene_bounds(void *h, float *bmin, float *bmax) {
    KdScene *r = (KdScene *)h;
    for (size_t i = 0; i < r->scene.prims.size(); ++i) {
        const B3 b = r->bvh.PrimWorldBound((uint32_t)i);
        for (int k = 0; k < 3; ++k) { bmin[3 * i + k] = b.pMin[k]; bmax[3 * i + k] = b.pMax[k]; }
    }
}
void kdref_scene_tree(void *h, uint32_t sizes[2], void *nodes8, uint32_t *idx) { SceneTree((const KdScene *)h, sizes, nodes8, idx); }
// rays with o[axis] == split
size_t kdref_scene_splits(void *h, int32_t *axis, float *pos, size_t cap) { return SceneSplits((const KdScene *)h, axis, pos, cap); }
void kdref_intersect(void *h, size_t n, const float *o, const float *d, const float *tmax, float *tOut, int32_t *primOut, float *bary,
                     uint64_t *counters4) {
    IntersectRays((const KdScene *)h, n, o, d, tmax, tOut, primOut, bary, counters4, 4);
}
void kdref_occluded(void *h, size_t n, const float *o, const float *d, const float *tmax, uint8_t *occ, uint64_t *counters4) {
    OccludedRays((const KdScene *)h, n, o, d, tmax, occ, counters4, 4);
}

}  // extern "C"
