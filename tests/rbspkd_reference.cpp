// Test-side restatement of the fork's kd-aware RBSP tree (accelerators/rbspKd.cpp with kDOPMesh.h, RBSPShared.h):
// RBSPKd::buildTree and the interior step of the two walks, Intersect and IntersectP, written independently of
// thesis-pbrt-v3_amd/csrc/ over the oracle's vector type and primitive tests (oracle/orc_accel.h, included read-only).  The k-DOP
// mesh, the direction sets, the walks and the scene plumbing are tests/tree_reference.h's, shared with the other tree
// accelerators' restatements.  The build follows the reference's own shape — a single-threaded scan with two running minima that
// keeps the best candidate's k-DOP halves — where the library costs candidates in parallel and cuts the winner again.  The walks
// count kd (direction < 3) and bsp interior nodes apart, and can be switched to the dot-product step of every node (RBSP's), the
// control that shows which rays tell the two interior forms apart.  Compiled with g++ at test time (tests/tree_ref.py), driven
// through ctypes.
#include "tree_reference.h"

namespace {

typedef TreeT<Node> Tree;

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

// RBSPKdNode::intersectInterior (rbspKd.cpp:69-92): planeDistance(split, ray, invDir, axis) at axis nodes, the direction's
// planeDistance (core/geometry.h:1833-1843) at oblique ones
struct RbspKdStep {
    typedef Node NodeT;
    bool dotOnly = false;          // the control: RBSP's dot-product step at every node, axis nodes included
    static uint32_t Shift(const Tree &t) { return BitOffset(t.M); }
    static uint32_t Axis(const Tree &t, const Node *n) { return n->flags & BitMask(t.M); }
    static bool IsLeaf(const Tree &t, const Node *n) { return (n->flags & BitMask(t.M)) == t.M; }
    static bool Kd(const Tree &t, const Node *n) { return (n->flags & BitMask(t.M)) < 3; }
    void Interior(const Tree &t, const Node *node, const Ray &ray, const V3 &invDir, Float *tPlane, bool *belowFirst) const {
        const uint32_t axis = node->flags & BitMask(t.M);
        if (axis < 3 && !dotOnly) {
            *tPlane = (node->split - ray.o[axis]) * invDir[axis];
            *belowFirst = (ray.o[axis] < node->split) || (ray.o[axis] == node->split && ray.d[axis] <= 0);
            return;
        }
        const V3 &dir = t.dirs[axis];
        const Float projectedO = Dot(dir, ray.o);
        const Float inverseProjectedD = 1 / Dot(dir, ray.d);
        *tPlane = (node->split - projectedO) * inverseProjectedD;
        *belowFirst = (projectedO < node->split) || (projectedO == node->split && inverseProjectedD <= 0);
    }
};
typedef SceneRef<RbspKdStep> RbspKdScene;

}  // namespace

extern "C" {

const char *rbspkdref_last_error() { return g_err.c_str(); }

// build over n triangles (9 floats each, creation order); sizes[0..1] = nodes, primitiveIndices entries
// returns null (rbspkdref_last_error) where the reference's build is undefined
void *rbspkdref_build(size_t n, const float *p9, int M, int isectCost, int travCost, int kdTravCost, float emptyBonus, int maxPrims, int maxDepth,
                      uint32_t sizes[2]) {
    Tree *t = new Tree();
    if (!Build(TrianglePrims(n, p9), (uint32_t)M, (uint32_t)isectCost, (uint32_t)travCost, (uint32_t)kdTravCost, emptyBonus, (uint32_t)maxPrims,
               (uint32_t)maxDepth, t)) {
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
    RbspKdScene *r = LoadSceneRef<RbspKdStep>(path);
    if (!r) return nullptr;
    r->tree.M = (uint32_t)M;
    r->tree.dirs = Directions((uint32_t)M);
    if (build && !Build(r->Prims(), (uint32_t)M, 80, 5, 1, 0.f, 1, (uint32_t)-1, &r->tree)) { g_err = "only the fixed-cost minimum is finite"; delete r; return nullptr; }
    return r;
}
void rbspkdref_scene_set_tree(void *h, int M, size_t nNodes, const void *nodes8, size_t nIdx, const uint32_t *idx) {
    RbspKdScene *r = (RbspKdScene *)h;
    r->tree.M = (uint32_t)M;
    r->tree.dirs = Directions((uint32_t)M);
    SceneSetTree(r, nNodes, nodes8, nIdx, idx);
}
size_t rbspkdref_scene_max_todo_dot(void *h, uint32_t *out) { return SceneMaxTodoDot((const RbspKdScene *)h, out); }
size_t rbspkdref_scene_max_todo(void *h, uint32_t *out) { return SceneMaxTodo((const RbspKdScene *)h, out); }
void rbspkdref_scene_free(void *h) { delete (RbspKdScene *)h; }
size_t rbspkdref_scene_prims(void *h) { return ((RbspKdScene *)h)->scene.prims.size(); }
size_t rbspkdref_scene_triangles(void *h, float *p9) { return SceneTriangles((const RbspKdScene *)h, p9); }
void rbspkdref_scene_tree(void *h, uint32_t sizes[2], void *nodes8, uint32_t *idx) { SceneTree((const RbspKdScene *)h, sizes, nodes8, idx); }
size_t rbspkdref_scene_splits(void *h, int32_t *axis, float *pos, size_t cap) { return SceneSplits((const RbspKdScene *)h, axis, pos, cap); }
// dot != 0: walk every interior node with the dot-product step (the control)
void rbspkdref_scene_dot_only(void *h, int dot) { ((RbspKdScene *)h)->step.dotOnly = dot != 0; }
// counters5: the fifth column is the kd interior nodes
void rbspkdref_intersect(void *h, size_t n, const float *o, const float *d, const float *tmax, float *tOut, int32_t *primOut, float *bary,
                         uint64_t *counters5) {
    IntersectRays((const RbspKdScene *)h, n, o, d, tmax, tOut, primOut, bary, counters5, 5);
}
void rbspkdref_occluded(void *h, size_t n, const float *o, const float *d, const float *tmax, uint8_t *occ, uint64_t *counters5) {
    OccludedRays((const RbspKdScene *)h, n, o, d, tmax, occ, counters5, 5);
}

}  // extern "C"
