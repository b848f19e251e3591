// Test-side restatement of the fork's kd-aware general BSP tree (accelerators/bspPaperKd.cpp, BSPKd.h, BSPKd.cpp):
// BSPPaperKd::buildTree and BSPKdNode::intersectInterior, the interior step of BSPKd::Intersect and BSPKd::IntersectP, written
// independently of thesis-pbrt-v3_amd/csrc/.  The k-DOP mesh, the walks and the scene plumbing are tests/tree_reference.h's; the
// k-DOP with its own directions, the triangles' planes, the node BVH with its two classifications and the build's working types
// are the general BSP tree's restatement's (tests/bsppaper_reference.cpp), which this file includes whole rather than repeat: both
// trees share them in the reference too (its bspref_* entry points come along unused).  The build follows the reference's own
// shape — a single-threaded scan with two running minima that keeps the best candidates' k-DOP halves — where the library costs
// candidates in parallel and cuts the winner again.  The walks count kd and plane interior nodes apart, and can be switched to
// the dot-product step at every node (a kd node then takes the unit axis its flags name), the control that shows which rays tell
// the two interior forms apart.  Compiled with g++ at test time (tests/tree_ref.py through tests/bsppaperkd_ref.py), driven
// through ctypes.
#include "bsppaper_reference.cpp"

namespace {

struct BSPKdNode {                  // BSPKdNode (BSPKd.h:163-173): 20 bytes
    union { float split; uint32_t onePrimitive; uint32_t primitiveIndicesOffset; };
    union { uint32_t flags; uint32_t nPrims; uint32_t aboveChild; };     // low 3 bits: 0-2 kd axis, 3 leaf, 4 plane node
    float splitAxis[3];
};
static_assert(sizeof(BSPKdNode) == 20, "BSPKdNode is 20 bytes");
typedef TreeT<BSPKdNode> KdAwareTree;

void BuildKd(const std::vector<Prim> &prims, uint32_t isectCost, uint32_t traversalCost, uint32_t kdTraversalCost, Float emptyBonus, uint32_t maxPrims,
             uint32_t maxDepth, KdAwareTree *tree) {
    const Float BSP_ALPHA = 0.1;
    const size_t N = prims.size();
    if (maxDepth == (uint32_t)-1) {
        const int lg = N ? 63 - __builtin_clzll((uint64_t)N) : -1;
        maxDepth = (uint32_t)std::round(2 + 1.6f * lg);
    }
    BvhScene bs(prims);
    tree->bounds = B3();
    for (const Prim &p : prims) tree->bounds = Union(tree->bounds, p.wb);
    DMesh root;
    {
        const B3 &b = tree->bounds;
        V3 v1 = b.pMin, v2(b.pMin.x, b.pMin.y, b.pMax.z), v3(b.pMin.x, b.pMax.y, b.pMin.z), v4(b.pMax.x, b.pMin.y, b.pMin.z);
        V3 v5(b.pMin.x, b.pMax.y, b.pMax.z), v6(b.pMax.x, b.pMin.y, b.pMax.z), v7(b.pMax.x, b.pMax.y, b.pMin.z), v8 = b.pMax;
        root.edges = {{v1, v2, 1, 3}, {v1, v3, 1, 5}, {v1, v4, 3, 5}, {v2, v5, 1, 4}, {v2, v6, 3, 4}, {v3, v5, 1, 2},
                      {v3, v7, 2, 5}, {v4, v6, 0, 3}, {v4, v7, 0, 5}, {v5, v8, 2, 4}, {v6, v8, 0, 4}, {v7, v8, 0, 2}};
        root.directions = {V3(1, 0, 0), V3(0, 1, 0), V3(0, 0, 1)};
    }
    const V3 kdDirections[3] = {V3(1, 0, 0), V3(0, 1, 0), V3(0, 0, 1)};
    std::vector<std::vector<BoundEdge>> edges(3, std::vector<BoundEdge>(2 * N));
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
        uint32_t bestK = (uint32_t)-1, bestOffset = (uint32_t)-1, bestKFixed = (uint32_t)-1;
        Float bestSplitT = 0, bestSplitTFixed = 0; V3 bestSplitAxis, bestSplitAxisFixed;
        std::pair<DMesh, DMesh> best, bestFixed;
        std::pair<Float, Float> bestAreas(0, 0), bestAreasFixed(0, 0);
        Float bestCost = Infinity, bestCostFixed = Infinity;
        const Float oldCost = isectCost * Float(cur.nPrimitives);
        const Float invTotalSA = 1 / cur.area;
        for (uint32_t k = 0; k < 3; ++k) {
            V3 d = kdDirections[k];
            Bnds db;
            for (auto &e : cur.mesh.edges) db = Union(db, e.getBounds(d));
            for (uint32_t i = 0; i < cur.nPrimitives; ++i) {
                const uint32_t pn = cur.primNums[i];
                edges[k][2 * i] = BoundEdge{prims[pn].wb.pMin[k], pn, EdgeType::Start};
                edges[k][2 * i + 1] = BoundEdge{prims[pn].wb.pMax[k], pn, EdgeType::End};
            }
            std::sort(&edges[k][0], &edges[k][0] + 2 * cur.nPrimitives, [](const BoundEdge &e0, const BoundEdge &e1) -> bool {
                if (e0.t == e1.t) return (int)e0.type < (int)e1.type;
                else return e0.t < e1.t;
            });
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
                    if (cost < bestCost) {
                        bestCost = cost; bestSplitT = edgeT; bestSplitAxis = d; bestK = k; bestOffset = i; best = cut;
                        bestAreas = std::make_pair(areaBelow, areaAbove);
                    }
                }
                if (edges[k][i].type == EdgeType::Start) ++nBelow;
            }
        }
        std::vector<PrimRef> plist(cur.nPrimitives);
        for (uint32_t i = 0; i < cur.nPrimitives; ++i) plist[i] = PrimRef{0, (int)cur.primNums[i]};
        NodeBvh nb{&prims, cur.primNums, BVH()};
        nb.bvh.Build(&bs.sc, &plist, nullptr, 0);
        for (uint32_t i = 0; i < cur.nPrimitives; ++i) {
            const uint32_t pn = cur.primNums[i];
            for (const Plane &plane : Planes(prims[pn])) {
                Bnds db;
                for (auto &e : cur.mesh.edges) db = Union(db, e.getBounds(plane.axis));
                if (plane.t > db.min && plane.t < db.max) {
                    std::pair<DMesh, DMesh> cut = cur.mesh.cut(plane.t, plane.axis);
                    const Float areaBelow = cut.first.SurfaceArea(), areaAbove = cut.second.SurfaceArea();
                    const Float pBelow = areaBelow * invTotalSA, pAbove = areaAbove * invTotalSA;
                    const std::pair<uint32_t, uint32_t> lr = nb.AmountToLeftAndRight(plane);
                    const Float eb = (lr.second == 0 || lr.first == 0) ? emptyBonus : 0;
                    const Float costIntersection = isectCost * (1 - eb) * (pBelow * lr.first + pAbove * lr.second);
                    const Float costFixed = traversalCost + costIntersection;
                    const Float cost = BSP_ALPHA * isectCost * (cur.nPrimitives - 1) + kdTraversalCost + costIntersection;
                    if (cost < bestCost) {
                        bestCost = cost; bestK = 33; bestSplitT = plane.t; bestSplitAxis = plane.axis; best = cut;
                        bestAreas = std::make_pair(areaBelow, areaAbove);
                    }
                    if (costFixed < bestCostFixed) {
                        bestCostFixed = costFixed; bestKFixed = 33; bestSplitTFixed = plane.t; bestSplitAxisFixed = plane.axis; bestFixed = cut;
                        bestAreasFixed = std::make_pair(areaBelow, areaAbove);
                    }
                }
            }
        }
        if (bestCost > oldCost && bestCostFixed > oldCost) ++cur.badRefines;
        if ((bestCost > 4 * oldCost && bestCostFixed > 4 * oldCost && cur.nPrimitives < 16) || (bestK == (uint32_t)-1 && bestKFixed == (uint32_t)-1) ||
            cur.badRefines == 3) {
            InitLeaf(nodeNum++, cur.primNums, cur.nPrimitives);
            continue;
        }
        uint32_t n0 = 0, n1 = 0;
        uint32_t *prims1 = cur.primNums, *prims0;
        if (bestK != (uint32_t)-1 && bestK != 33) {
            for (uint32_t i = bestOffset + 1; i < 2 * cur.nPrimitives; ++i)
                if (edges[bestK][i].type == EdgeType::End) prims1[n1++] = edges[bestK][i].primNum;
            prims0 = prims1 + n1;
            for (uint32_t i = 0; i < bestOffset; ++i)
                if (edges[bestK][i].type == EdgeType::Start) prims0[n0++] = edges[bestK][i].primNum;
        } else {
            std::vector<uint32_t> left, right;
            if (bestK != (uint32_t)-1) nb.PrimnumsToLeftAndRight(Plane{bestSplitT, bestSplitAxis}, left, right);
            else nb.PrimnumsToLeftAndRight(Plane{bestSplitTFixed, bestSplitAxisFixed}, left, right);
            for (uint32_t &x : left) x = cur.primNums[x];
            for (uint32_t &x : right) x = cur.primNums[x];
            for (uint32_t x : right) prims1[n1++] = x;
            prims0 = prims1 + n1;
            for (uint32_t x : left) prims0[n0++] = x;
        }
        auto InitInterior = [&](const V3 &axis, Float s) {      // BSPKd.h:40-44
            nodes[nodeNum].split = s;
            nodes[nodeNum].splitAxis[0] = axis.x; nodes[nodeNum].splitAxis[1] = axis.y; nodes[nodeNum].splitAxis[2] = axis.z;
            nodes[nodeNum].flags = 4;
        };
        if (bestK != (uint32_t)-1) {
            if (bestK == 33) InitInterior(bestSplitAxis, bestSplitT);
            else { nodes[nodeNum].split = bestSplitT; nodes[nodeNum].flags = bestK; }      // initInteriorKd: splitAxis stays unset (here zero)
            stack.push_back(BuildNode{cur.depth - 1, n1, cur.badRefines, best.second, bestAreas.second, prims1, nodeNum});
            stack.push_back(BuildNode{cur.depth - 1, n0, cur.badRefines, best.first, bestAreas.first, prims0, (uint32_t)-1});
        } else {
            InitInterior(bestSplitAxisFixed, bestSplitTFixed);
            stack.push_back(BuildNode{cur.depth - 1, n1, cur.badRefines, bestFixed.second, bestAreasFixed.second, prims1, nodeNum});
            stack.push_back(BuildNode{cur.depth - 1, n0, cur.badRefines, bestFixed.first, bestAreasFixed.first, prims0, (uint32_t)-1});
        }
        ++nodeNum;
    }
}

// BSPKdNode::intersectInterior (BSPKd.h:59-83): planeDistance(split, ray, invDir, axis) at kd nodes, the axis's planeDistance
// (core/geometry.h:1837-1843) at plane nodes
struct BspKdStep {
    typedef BSPKdNode NodeT;
    bool dotOnly = false;          // the control: the dot-product step at every node, a kd node over the unit axis it names
    static uint32_t Shift(const KdAwareTree &) { return 3; }
    static bool IsLeaf(const KdAwareTree &, const BSPKdNode *n) { return (n->flags & 7u) == 3u; }
    static bool Kd(const KdAwareTree &, const BSPKdNode *n) { return (n->flags & 7u) < 4u; }      // isKdNode, asked of interior nodes only
    void Interior(const KdAwareTree &, const BSPKdNode *node, const Ray &ray, const V3 &invDir, Float *tPlane, bool *belowFirst) const {
        const bool kd = (node->flags & 7u) < 4u;
        const uint32_t a = node->flags & 7u;
        if (kd && !dotOnly) {
            *tPlane = (node->split - ray.o[a]) * invDir[a];
            *belowFirst = (ray.o[a] < node->split) || (ray.o[a] == node->split && ray.d[a] <= 0);
            return;
        }
        const V3 axis = kd ? V3(a == 0 ? 1.f : 0.f, a == 1 ? 1.f : 0.f, a == 2 ? 1.f : 0.f) : V3(node->splitAxis[0], node->splitAxis[1], node->splitAxis[2]);
        const Float projectedO = Dot(axis, ray.o);
        const Float inverseProjectedD = 1 / Dot(axis, ray.d);
        *tPlane = (node->split - projectedO) * inverseProjectedD;
        *belowFirst = (projectedO < node->split) || (projectedO == node->split && inverseProjectedD <= 0);
    }
};
typedef SceneRef<BspKdStep> BspKdScene;

}  // namespace

extern "C" {

const char *bspkdref_last_error() { return g_err.c_str(); }

// build over n triangles (9 floats each, creation order); sizes[0..1] = nodes, primitiveIndices entries
void *bspkdref_build(size_t n, const float *p9, int isectCost, int travCost, int kdTravCost, float emptyBonus, int maxPrims, int maxDepth,
                     uint32_t sizes[2]) {
    KdAwareTree *t = new KdAwareTree();
    BuildKd(TrianglePrims(n, p9), (uint32_t)isectCost, (uint32_t)travCost, (uint32_t)kdTravCost, emptyBonus, (uint32_t)maxPrims, (uint32_t)maxDepth, t);
    sizes[0] = (uint32_t)t->nodes.size(); sizes[1] = (uint32_t)t->primitiveIndices.size();
    return t;
}
// nodes20: 5 words per node (the axis words of kd nodes and leaves zero)
void bspkdref_copy(void *h, void *nodes20, uint32_t *idx) { CopyTree(*(const KdAwareTree *)h, nodes20, idx, nullptr); }
void bspkdref_free(void *h) { delete (KdAwareTree *)h; }

// a baked scene (no instances) and its BVH (for the ordered numbering); build != 0: the restated default tree, else set_tree
void *bspkdref_scene_load(const char *path, int build) {
    BspKdScene *r = LoadSceneRef<BspKdStep>(path);
    if (r && build) BuildKd(r->Prims(), 80, 5, 1, 0.f, 1, (uint32_t)-1, &r->tree);
    return r;
}
void bspkdref_scene_set_tree(void *h, size_t nNodes, const void *nodes20, size_t nIdx, const uint32_t *idx) { SceneSetTree((BspKdScene *)h, nNodes, nodes20, nIdx, idx); }
size_t bspkdref_scene_max_todo(void *h, uint32_t *out) { return SceneMaxTodo((const BspKdScene *)h, out); }
void bspkdref_scene_free(void *h) { delete (BspKdScene *)h; }
size_t bspkdref_scene_prims(void *h) { return ((BspKdScene *)h)->scene.prims.size(); }
size_t bspkdref_scene_triangles(void *h, float *p9) { return SceneTriangles((const BspKdScene *)h, p9); }
void bspkdref_scene_tree(void *h, uint32_t sizes[2], void *nodes20, uint32_t *idx) { SceneTree((const BspKdScene *)h, sizes, nodes20, idx); }
// dot != 0: walk every interior node with the dot-product step (the control)
void bspkdref_scene_dot_only(void *h, int dot) { ((BspKdScene *)h)->step.dotOnly = dot != 0; }
// counters5: the fifth column is the kd interior nodes
void bspkdref_intersect(void *h, size_t n, const float *o, const float *d, const float *tmax, float *tOut, int32_t *primOut, float *bary,
                        uint64_t *counters5) {
    IntersectRays((const BspKdScene *)h, n, o, d, tmax, tOut, primOut, bary, counters5, 5);
}
void bspkdref_occluded(void *h, size_t n, const float *o, const float *d, const float *tmax, uint8_t *occ, uint64_t *counters5) {
    OccludedRays((const BspKdScene *)h, n, o, d, tmax, occ, counters5, 5);
}

}  // extern "C"
