// Test-side restatement of the fork's RBSP tree (accelerators/rbsp.cpp, kDOPMesh.h, RBSPShared.h): RBSP::buildTree and the
// interior step of the two walks, Intersect and IntersectP, written independently of thesis-pbrt-v3_amd/csrc/ over the oracle's
// vector type and primitive tests (oracle/orc_accel.h, included read-only).  The k-DOP mesh, the direction sets, the walks and the
// scene plumbing are tests/tree_reference.h's, shared with the other tree accelerators' restatements.  The build follows the
// reference's own shape — a single-threaded scan that keeps the best candidate's k-DOP halves, meshes as vectors of edges, faces
// as vectors of edge pointers — where the library costs candidates in parallel and cuts the winner again.  Compiled with g++ at
// test time (tests/tree_ref.py), driven through ctypes.  It pins nothing against a reference binary: the device walk is held to
// THIS walk ("parity unpinned").
#include "tree_reference.h"

namespace {

typedef TreeT<Node> Tree;

enum class EdgeType { Start, End };
struct BoundEdge { Float t; uint32_t primNum; EdgeType type; };
struct BuildNode { uint32_t depth, nPrimitives, badRefines; std::vector<Bnds> nodeBounds; KMesh mesh; Float area; uint32_t *primNums; uint32_t parentNum; };

void Build(const std::vector<Prim> &prims, uint32_t M, uint32_t isectCost, uint32_t traversalCost, Float emptyBonus, uint32_t maxPrims,
           uint32_t maxDepth, Tree *tree) {
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
        uint32_t bestD = (uint32_t)-1, bestOffset = (uint32_t)-1;
        std::pair<KMesh, KMesh> best;
        std::pair<Float, Float> bestAreas(0, 0);
        Float bestCost = Infinity;
        const Float oldCost = isectCost * Float(cur.nPrimitives);
        const Float invTotalSA = 1 / cur.area;
        for (uint32_t d = 0; d < M; ++d) {
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
                    const Float cost = traversalCost + isectCost * (1 - eb) * (pBelow * nBelow + pAbove * nAbove);
                    if (cost < bestCost) { bestCost = cost; bestD = d; bestOffset = i; best = cut; bestAreas = std::make_pair(areaBelow, areaAbove); }
                }
                if (edges[d][i].type == EdgeType::Start) ++nBelow;
            }
        }
        if (bestCost > oldCost) ++cur.badRefines;
        if ((bestCost > 4 * oldCost && cur.nPrimitives < 16) || bestD == (uint32_t)-1 || cur.badRefines == 3) {
            InitLeaf(nodeNum++, cur.primNums, cur.nPrimitives);
            continue;
        }
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
}

// RBSPNode: the direction in the low BitOffset(M) bits, M a leaf; intersectInterior with planeDistance (core/geometry.h:1837-1843)
struct RbspStep {
    typedef Node NodeT;
    static uint32_t Shift(const Tree &t) { return BitOffset(t.M); }
    static uint32_t Axis(const Tree &t, const Node *n) { return n->flags & BitMask(t.M); }
    static bool IsLeaf(const Tree &t, const Node *n) { return (n->flags & BitMask(t.M)) == t.M; }
    static bool Kd(const Tree &, const Node *) { return false; }       // (only rbspkd counts its axis nodes apart)
    static void Interior(const Tree &t, const Node *node, const Ray &ray, const V3 &, Float *tPlane, bool *belowFirst) {
        const V3 &dir = t.dirs[node->flags & BitMask(t.M)];
        const Float projectedO = Dot(dir, ray.o);
        const Float inverseProjectedD = 1 / Dot(dir, ray.d);
        *tPlane = (node->split - projectedO) * inverseProjectedD;
        *belowFirst = (projectedO < node->split) || (projectedO == node->split && inverseProjectedD <= 0);
    }
};
typedef SceneRef<RbspStep> RbspScene;

}  // namespace

extern "C" {

const char *rbspref_last_error() { return g_err.c_str(); }

// build over n triangles (9 floats each, creation order); sizes[0..1] = nodes, primitiveIndices entries
void *rbspref_build(size_t n, const float *p9, int M, int isectCost, int travCost, float emptyBonus, int maxPrims, int maxDepth, uint32_t sizes[2]) {
    Tree *t = new Tree();
    Build(TrianglePrims(n, p9), (uint32_t)M, (uint32_t)isectCost, (uint32_t)travCost, emptyBonus, (uint32_t)maxPrims, (uint32_t)maxDepth, t);
    sizes[0] = (uint32_t)t->nodes.size(); sizes[1] = (uint32_t)t->primitiveIndices.size();
    return t;
}
void rbspref_copy(void *h, void *nodes8, uint32_t *idx, float *dirs) { CopyTree(*(const Tree *)h, nodes8, idx, dirs); }
void rbspref_free(void *h) { delete (Tree *)h; }

// a baked scene (no instances) and its BVH (for the ordered numbering).  build != 0: the restated tree over its primitives
// with nbDirections M and the other defaults; else the tree is given with rbspref_scene_set_tree.
void *rbspref_scene_load(const char *path, int M, int build) {
    RbspScene *r = LoadSceneRef<RbspStep>(path);
    if (!r) return nullptr;
    r->tree.M = (uint32_t)M;
    r->tree.dirs = Directions((uint32_t)M);
    if (build) Build(r->Prims(), (uint32_t)M, 80, 5, 0.f, 1, (uint32_t)-1, &r->tree);
    return r;
}
void rbspref_scene_set_tree(void *h, int M, size_t nNodes, const void *nodes8, size_t nIdx, const uint32_t *idx) {
    RbspScene *r = (RbspScene *)h;
    r->tree.M = (uint32_t)M;
    r->tree.dirs = Directions((uint32_t)M);
    SceneSetTree(r, nNodes, nodes8, nIdx, idx);
}
size_t rbspref_scene_max_todo(void *h, uint32_t *out) { return SceneMaxTodo((const RbspScene *)h, out); }
void rbspref_scene_free(void *h) { delete (RbspScene *)h; }
size_t rbspref_scene_prims(void *h) { return ((RbspScene *)h)->scene.prims.size(); }
size_t rbspref_scene_triangles(void *h, float *p9) { return SceneTriangles((const RbspScene *)h, p9); }
void rbspref_scene_tree(void *h, uint32_t sizes[2], void *nodes8, uint32_t *idx) { SceneTree((const RbspScene *)h, sizes, nodes8, idx); }
size_t rbspref_scene_splits(void *h, int32_t *axis, float *pos, size_t cap) { return SceneSplits((const RbspScene *)h, axis, pos, cap); }
void rbspref_intersect(void *h, size_t n, const float *o, const float *d, const float *tmax, float *tOut, int32_t *primOut, float *bary,
                       uint64_t *counters4) {
    IntersectRays((const RbspScene *)h, n, o, d, tmax, tOut, primOut, bary, counters4, 4);
}
void rbspref_occluded(void *h, size_t n, const float *o, const float *d, const float *tmax, uint8_t *occ, uint64_t *counters4) {
    OccludedRays((const RbspScene *)h, n, o, d, tmax, occ, counters4, 4);
}

}  // extern "C"
