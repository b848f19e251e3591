// Test-side restatement of the fork's general BSP tree (accelerators/bspPaper.cpp, BSP.h, BSP.cpp, kDOPMesh.h, bvh.cpp:439-527,
// shapes/triangle.cpp:584-594 and 678-720): BSPPaper::buildTree and the interior step of the two walks, BSP::Intersect and
// BSP::IntersectP, written independently of thesis-pbrt-v3_amd/csrc/ over the oracle's vector type, BVH builder and primitive
// tests (oracle/orc_accel.h, included read-only).  The k-DOP mesh, the walks and the scene plumbing are tests/tree_reference.h's,
// shared with the other tree accelerators' restatements.  The build follows the reference's own shape — a single-threaded scan
// that keeps the best candidate's k-DOP halves, a k-DOP that carries its own direction list, the node's BVH built by the oracle's
// BVHAccel restatement — where the library costs candidates in parallel and cuts the winner again.  Compiled with g++ at test
// time (tests/tree_ref.py), driven through ctypes.
// It pins nothing against a reference binary: the device walk is held to THIS walk ("parity unpinned").
#include "tree_reference.h"

namespace {

struct BSPNode {                    // BSPNode (BSP.h:122-184): 20 bytes
    union { float split; uint32_t onePrimitive; uint32_t primitiveIndicesOffset; };
    union { uint32_t flags; uint32_t nPrims; uint32_t aboveChild; };
    float splitAxis[3];
};
static_assert(sizeof(BSPNode) == 20, "BSPNode is 20 bytes");

// KDOPMeshWithDirections (kDOPMesh.h:238-266)
struct DMesh {
    std::vector<KEdge> edges;
    std::vector<V3> directions;
    std::pair<DMesh, DMesh> cut(Float t, const V3 &direction) const {
        uint32_t directionId = (uint32_t)directions.size();
        for (uint32_t i = 0; i < directions.size(); i++)
            if (Dot(directions[i], direction) > 0.999961923) { directionId = i; break; }
        std::pair<KMesh, KMesh> c = CutMesh(edges, (uint32_t)directions.size(), t, direction, directionId);
        std::pair<DMesh, DMesh> r;
        r.first.edges = c.first.edges; r.second.edges = c.second.edges;
        r.first.directions = directions; r.second.directions = directions;
        if (directionId == directions.size()) { r.first.directions.push_back(direction); r.second.directions.push_back(direction); }
        return r;
    }
    Float SurfaceArea() { return MeshArea(edges, directions); }
};

struct Plane { Float t; V3 axis; };

// PositiveX (core/geometry.h:1849-1862)
V3 PositiveX(V3 v) {
    if (v.x > 0) return Normalize(v);
    if (v.x == 0) {
        if (v.y == 0) return Normalize(V3(0, 0, 1));
        return Normalize(V3(0, v.y / ((v.y > 0) ? 1 : -1), v.z / ((v.y > 0) ? 1 : -1)));
    }
    return Normalize(V3(-v.x, -v.y, -v.z));
}

// Triangle::Normal (shapes/triangle.cpp:584-594) and getBSPPaperPlanes (:678-720)
std::vector<Plane> Planes(const Prim &pr) {
    std::vector<Plane> planes;
    if (!pr.tri) return planes;
    const V3 &p0 = pr.p[0], &p1 = pr.p[1], &p2 = pr.p[2];
    V3 n = Cross(p0 - p2, p1 - p2);
    if (n.Length() > 0) n = Normalize(n);
    if (n.Length() > 0) {
        n = PositiveX(n);
        planes.push_back(Plane{Dot(n, p0), n});
        V3 axis = Cross(n, p0 - p1);
        if (axis.Length() > 0) { axis = PositiveX(axis); planes.push_back(Plane{Dot(axis, p0), axis}); }
        axis = Cross(n, p0 - p2);
        if (axis.Length() > 0) { axis = PositiveX(axis); planes.push_back(Plane{Dot(axis, p0), axis}); }
        axis = Cross(n, p1 - p2);
        if (axis.Length() > 0) { axis = PositiveX(axis); planes.push_back(Plane{Dot(axis, p1), axis}); }
    }
    return planes;
}

// Primitive::getBounds(direction): Triangle::getBounds or the world bound's corners (core/shape.h:103-113)
Bnds GetBounds(const Prim &p, const V3 &d) {
    Bnds b;
    if (p.tri) {
        Float t = Dot(d, p.p[0]);
        Float mn = t, mx = t;
        for (int k = 1; k < 3; ++k) { t = Dot(d, p.p[k]); if (t > mx) mx = t; else if (t < mn) mn = t; }
        b.min = mn; b.max = mx;
    } else {
        for (int c = 0; c < 8; ++c) {
            const V3 q((c & 1) ? p.wb.pMax.x : p.wb.pMin.x, (c & 2) ? p.wb.pMax.y : p.wb.pMin.y, (c & 4) ? p.wb.pMax.z : p.wb.pMin.z);
            const float proj = Dot(d, q);
            if (proj < b.min) b.min = proj;
            if (proj > b.max) b.max = proj;
        }
    }
    return b;
}

// BVHAccel(currentPrimitives, 4, 8, 1) over a node's primitives, built by the oracle's restatement (its scene stands in for the
// primitives' shapes: one mesh of the triangles), and the two classifications (bvh.cpp:439-527)
struct NodeBvh {
    const std::vector<Prim> *prims; const uint32_t *primNums;     // local i -> global primNums[i]
    BVH bvh;
    Bnds LeafBounds(uint32_t ordered, const Plane &p) const { return GetBounds((*prims)[primNums[bvh.primOrder[ordered]]], p.axis); }
    void Center(const LinearBVHNode &nd, Float *maxDiff, Float *cp, const Plane &p) const {
        const V3 lo(nd.bmin[0], nd.bmin[1], nd.bmin[2]), hi(nd.bmax[0], nd.bmax[1], nd.bmax[2]);
        const V3 diag = hi - lo;
        *maxDiff = diag.Length() / 2;
        const V3 center = lo + diag / 2;
        *cp = Dot(p.axis, center);
    }
    std::pair<uint32_t, uint32_t> AmountToLeftAndRight(const Plane &p) const {
        uint32_t left = 0, right = 0;
        std::vector<uint32_t> stack{0};
        while (!stack.empty()) {
            const uint32_t cur = stack.back(); stack.pop_back();
            const LinearBVHNode *node = &bvh.nodes[cur];
            Float maxDiff, cp; Center(*node, &maxDiff, &cp, p);
            if (cp + maxDiff < p.t) left += node->nPrimitives();
            else if (cp - maxDiff > p.t) right += node->nPrimitives();
            else if (node->IsLeaf()) {
                for (uint32_t i = 0; i < node->nPrimitives(); ++i) {
                    const Bnds b = LeafBounds(node->offset + i, p);
                    if (b.min <= p.t) left += 1;
                    if (b.max >= p.t) right += 1;
                }
            } else { stack.push_back(cur + 1); stack.push_back(node->offset); }
        }
        return std::make_pair(left, right);
    }
    void PrimnumsToLeftAndRight(const Plane &p, std::vector<uint32_t> &left, std::vector<uint32_t> &right) const {
        std::vector<std::pair<uint32_t, uint8_t>> stack{{0u, (uint8_t)0}};
        while (!stack.empty()) {
            const std::pair<uint32_t, uint8_t> cur = stack.back(); stack.pop_back();
            const LinearBVHNode *node = &bvh.nodes[cur.first];
            auto all = [&](std::vector<uint32_t> &out) { for (uint32_t i = 0; i < node->nPrimitives(); ++i) out.push_back(bvh.primOrder[node->offset + i]); };
            if (cur.second == 0) {
                Float maxDiff, cp; Center(*node, &maxDiff, &cp, p);
                if (cp + maxDiff < p.t) {
                    if (node->IsLeaf()) all(left);
                    else { stack.push_back({cur.first + 1, 1}); stack.push_back({(uint32_t)node->offset, 1}); }
                } else if (cp - maxDiff > p.t) {
                    if (node->IsLeaf()) all(right);
                    else { stack.push_back({cur.first + 1, 2}); stack.push_back({(uint32_t)node->offset, 2}); }
                } else if (node->IsLeaf()) {
                    for (uint32_t i = 0; i < node->nPrimitives(); ++i) {
                        const Bnds b = LeafBounds(node->offset + i, p);
                        if (b.min <= p.t) left.push_back(bvh.primOrder[node->offset + i]);
                        if (b.max >= p.t) right.push_back(bvh.primOrder[node->offset + i]);
                    }
                } else { stack.push_back({cur.first + 1, 0}); stack.push_back({(uint32_t)node->offset, 0}); }
            } else if (node->IsLeaf()) {
                if (cur.second == 1) all(left); else all(right);
            } else { stack.push_back({cur.first + 1, cur.second}); stack.push_back({(uint32_t)node->offset, cur.second}); }
        }
    }
};

// The oracle BVH builds over a Scene: one mesh holding every primitive's triangle (or a degenerate stand-in whose world bound is
// the primitive's), with the BVH parameters of the per-node BVHAccel
struct BvhScene {
    Scene sc;
    explicit BvhScene(const std::vector<Prim> &prims) {
        sc.prm = SceneParams();
        sc.prm.maxNodePrims = 1; sc.prm.isectCost = 4; sc.prm.travCost = 8;
        Mesh m;
        m.nTris = (uint32_t)prims.size(); m.nVerts = 3 * m.nTris; m.hasN = m.hasUV = m.hasS = false;
        for (size_t i = 0; i < prims.size(); ++i) {
            const Prim &p = prims[i];
            if (p.tri) for (int k = 0; k < 3; ++k) m.p.push_back(p.p[k]);
            else { m.p.push_back(p.wb.pMin); m.p.push_back(p.wb.pMax); m.p.push_back(p.wb.pMin); }
            for (int k = 0; k < 3; ++k) m.idx.push_back((int)(3 * i + k));
        }
        sc.meshes.push_back(m);
        ShapeRec s{};
        s.kind = SHAPE_MESH; s.meshIndex = 0; s.nPrims = m.nTris;
        sc.shapes.push_back(s);
    }
};

typedef TreeT<BSPNode> Tree;

enum class EdgeType { Start, End };
struct BoundEdge { Float t; uint32_t primNum; EdgeType type; };
struct BuildNode { uint32_t depth, nPrimitives, badRefines; DMesh mesh; Float area; uint32_t *primNums; uint32_t parentNum; };

void Build(const std::vector<Prim> &prims, uint32_t isectCost, uint32_t traversalCost, Float emptyBonus, uint32_t maxPrims, uint32_t maxDepth,
           Tree *tree) {
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
        Float bestSplitT = 0; V3 bestSplitAxis;
        std::pair<DMesh, DMesh> best;
        std::pair<Float, Float> bestAreas(0, 0);
        Float bestCost = Infinity;
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
                    const Float cost = traversalCost + isectCost * (1 - eb) * (pBelow * nBelow + pAbove * nAbove);
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
                    const Float cost = traversalCost + isectCost * (1 - eb) * (pBelow * lr.first + pAbove * lr.second);
                    if (cost < bestCost) {
                        bestCost = cost; bestK = 33; bestSplitT = plane.t; bestSplitAxis = plane.axis; best = cut;
                        bestAreas = std::make_pair(areaBelow, areaAbove);
                    }
                }
            }
        }
        if (bestCost > oldCost) ++cur.badRefines;
        if ((bestCost > 4 * oldCost && cur.nPrimitives < 16) || bestK == (uint32_t)-1 || cur.badRefines == 3) {
            InitLeaf(nodeNum++, cur.primNums, cur.nPrimitives);
            continue;
        }
        uint32_t n0 = 0, n1 = 0;
        uint32_t *prims1 = cur.primNums, *prims0;
        if (bestK != 33) {
            for (uint32_t i = bestOffset + 1; i < 2 * cur.nPrimitives; ++i)
                if (edges[bestK][i].type == EdgeType::End) prims1[n1++] = edges[bestK][i].primNum;
            prims0 = prims1 + n1;
            for (uint32_t i = 0; i < bestOffset; ++i)
                if (edges[bestK][i].type == EdgeType::Start) prims0[n0++] = edges[bestK][i].primNum;
        } else {
            std::vector<uint32_t> left, right;
            nb.PrimnumsToLeftAndRight(Plane{bestSplitT, bestSplitAxis}, left, right);
            for (uint32_t &x : left) x = cur.primNums[x];
            for (uint32_t &x : right) x = cur.primNums[x];
            for (uint32_t x : right) prims1[n1++] = x;
            prims0 = prims1 + n1;
            for (uint32_t x : left) prims0[n0++] = x;
        }
        nodes[nodeNum].split = bestSplitT;
        nodes[nodeNum].splitAxis[0] = bestSplitAxis.x; nodes[nodeNum].splitAxis[1] = bestSplitAxis.y; nodes[nodeNum].splitAxis[2] = bestSplitAxis.z;
        nodes[nodeNum].flags = 0;
        stack.push_back(BuildNode{cur.depth - 1, n1, cur.badRefines, best.second, bestAreas.second, prims1, nodeNum});
        stack.push_back(BuildNode{cur.depth - 1, n0, cur.badRefines, best.first, bestAreas.first, prims0, (uint32_t)-1});
        ++nodeNum;
    }
}

// BSPNode: the low bit a leaf; treeIntersectInterior with planeDistance (BSP.h:66-78, core/geometry.h:1837-1843)
struct BspStep {
    typedef BSPNode NodeT;
    static uint32_t Shift(const Tree &) { return 1; }
    static bool IsLeaf(const Tree &, const BSPNode *n) { return (n->flags & 1u) == 1u; }
    static bool Kd(const Tree &, const BSPNode *) { return false; }    // (only rbspkd counts its axis nodes apart)
    static void Interior(const Tree &, const BSPNode *node, const Ray &ray, const V3 &, Float *tPlane, bool *belowFirst) {
        const V3 axis(node->splitAxis[0], node->splitAxis[1], node->splitAxis[2]);
        const Float projectedO = Dot(axis, ray.o);
        const Float inverseProjectedD = 1 / Dot(axis, ray.d);
        *tPlane = (node->split - projectedO) * inverseProjectedD;
        *belowFirst = (projectedO < node->split) || (projectedO == node->split && inverseProjectedD <= 0);
    }
};
typedef SceneRef<BspStep> BspScene;

}  // namespace

extern "C" {

const char *bspref_last_error() { return g_err.c_str(); }

// build over n triangles (9 floats each, creation order); sizes[0..1] = nodes, primitiveIndices entries
void *bspref_build(size_t n, const float *p9, int isectCost, int travCost, float emptyBonus, int maxPrims, int maxDepth, uint32_t sizes[2]) {
    Tree *t = new Tree();
    Build(TrianglePrims(n, p9), (uint32_t)isectCost, (uint32_t)travCost, emptyBonus, (uint32_t)maxPrims, (uint32_t)maxDepth, t);
    sizes[0] = (uint32_t)t->nodes.size(); sizes[1] = (uint32_t)t->primitiveIndices.size();
    return t;
}
// nodes20: 5 words per node (leaves' axis words zero)
void bspref_copy(void *h, void *nodes20, uint32_t *idx) { CopyTree(*(const Tree *)h, nodes20, idx, nullptr); }
void bspref_free(void *h) { delete (Tree *)h; }
// getBSPPaperPlanes of one triangle: planes4[4 k ..] = {t, axis}; returns how many
size_t bspref_planes(const float *p9, float *planes4) {
    const std::vector<Plane> pl = Planes(TrianglePrims(1, p9)[0]);
    for (size_t k = 0; k < pl.size(); ++k) { planes4[4 * k] = pl[k].t; planes4[4 * k + 1] = pl[k].axis.x; planes4[4 * k + 2] = pl[k].axis.y; planes4[4 * k + 3] = pl[k].axis.z; }
    return pl.size();
}
// the two BVH classifications over n triangles (a BVH over all of them, isectCost 4, travCost 8, maxPrims 1); sizes: left / right lengths
void bspref_classify(size_t n, const float *p9, const float *plane4, uint32_t counts[2], uint32_t *left, uint32_t *right, size_t cap, uint32_t sizes[2]) {
    const std::vector<Prim> prims = TrianglePrims(n, p9);
    BvhScene bs(prims);
    std::vector<uint32_t> ident(n);
    std::vector<PrimRef> plist(n);
    for (size_t i = 0; i < n; ++i) { ident[i] = (uint32_t)i; plist[i] = PrimRef{0, (int)i}; }
    NodeBvh nb{&prims, ident.data(), BVH()};
    nb.bvh.Build(&bs.sc, &plist, nullptr, 0);
    const Plane p{plane4[0], V3(plane4[1], plane4[2], plane4[3])};
    const std::pair<uint32_t, uint32_t> lr = nb.AmountToLeftAndRight(p);
    counts[0] = lr.first; counts[1] = lr.second;
    std::vector<uint32_t> l, r;
    nb.PrimnumsToLeftAndRight(p, l, r);
    sizes[0] = (uint32_t)l.size(); sizes[1] = (uint32_t)r.size();
    for (size_t k = 0; k < l.size() && k < cap; ++k) left[k] = l[k];
    for (size_t k = 0; k < r.size() && k < cap; ++k) right[k] = r[k];
}

// a baked scene (no instances) and its BVH (for the ordered numbering); build != 0: the restated default tree, else set_tree
void *bspref_scene_load(const char *path, int build) {
    BspScene *r = LoadSceneRef<BspStep>(path);
    if (r && build) Build(r->Prims(), 80, 5, 0.f, 1, (uint32_t)-1, &r->tree);
    return r;
}
void bspref_scene_set_tree(void *h, size_t nNodes, const void *nodes20, size_t nIdx, const uint32_t *idx) { SceneSetTree((BspScene *)h, nNodes, nodes20, nIdx, idx); }
size_t bspref_scene_max_todo(void *h, uint32_t *out) { return SceneMaxTodo((const BspScene *)h, out); }
void bspref_scene_free(void *h) { delete (BspScene *)h; }
size_t bspref_scene_prims(void *h) { return ((BspScene *)h)->scene.prims.size(); }
size_t bspref_scene_triangles(void *h, float *p9) { return SceneTriangles((const BspScene *)h, p9); }
void bspref_scene_tree(void *h, uint32_t sizes[2], void *nodes20, uint32_t *idx) { SceneTree((const BspScene *)h, sizes, nodes20, idx); }
void bspref_intersect(void *h, size_t n, const float *o, const float *d, const float *tmax, float *tOut, int32_t *primOut, float *bary,
                      uint64_t *counters4) {
    IntersectRays((const BspScene *)h, n, o, d, tmax, tOut, primOut, bary, counters4, 4);
}
void bspref_occluded(void *h, size_t n, const float *o, const float *d, const float *tmax, uint8_t *occ, uint64_t *counters4) {
    OccludedRays((const BspScene *)h, n, o, d, tmax, occ, counters4, 4);
}

}  // extern "C"
