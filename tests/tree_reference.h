// What the test-side restatements of the fork's tree accelerators share (tests/{kd,rbsp,rbspkd,bsppaper}_reference.cpp): the
// 8-byte node, the k-DOP mesh (kDOPMesh.h) and the direction sets (RBSPShared.h), the root interval, the two todo-list walks as
// templates over an accelerator's interior step (the test-side counterpart of csrc/device/bsp_walk.h's Step), the scene
// plumbing and the marshalling of rays and results.  Written independently of thesis-pbrt-v3_amd/csrc/ over the oracle's vector
// type, BVH and primitive tests (oracle/orc_accel.h, included read-only): it includes nothing of the code under test.  Each
// restatement is one translation unit that includes this header once and adds its own Build, step and extern "C" names.
#pragma once
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

struct Node {                       // KdAccelNode / RBSPNode: union { split, onePrimitive, primitiveIndicesOffset }; union { flags, nPrims, aboveChild }
    union { float split; uint32_t onePrimitive; uint32_t primitiveIndicesOffset; };
    union { uint32_t flags; uint32_t nPrims; uint32_t aboveChild; };
};
static_assert(sizeof(Node) == 8, "KdAccelNode and RBSPNode are 8 bytes");

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

// A primitive as the builders over triangles see it: a triangle's three world vertices, or (tri == false) a world bound
struct Prim { bool tri; V3 p[3]; B3 wb; };

std::vector<Prim> TrianglePrims(size_t n, const float *p9) {
    std::vector<Prim> prims(n);
    for (size_t i = 0; i < n; ++i) {
        Prim &p = prims[i];
        p.tri = true;
        for (int k = 0; k < 3; ++k) p.p[k] = V3(p9[9 * i + 3 * k], p9[9 * i + 3 * k + 1], p9[9 * i + 3 * k + 2]);
        p.wb = Union(B3(p.p[0], p.p[1]), p.p[2]);
    }
    return prims;
}

// M, dirs: the direction set of the RBSP family (kd and bsppaper leave them alone)
template <class NodeT> struct TreeT {
    uint32_t M = 3;
    std::vector<V3> dirs;
    std::vector<NodeT> nodes;
    std::vector<uint32_t> primitiveIndices;
    B3 bounds;
};

template <class NodeT> void CopyTree(const TreeT<NodeT> &t, void *nodes, uint32_t *idx, float *dirs) {
    if (nodes) memcpy(nodes, t.nodes.data(), t.nodes.size() * sizeof(NodeT));
    if (idx && !t.primitiveIndices.empty()) memcpy(idx, t.primitiveIndices.data(), t.primitiveIndices.size() * 4);
    if (dirs) for (size_t k = 0; k < t.dirs.size(); ++k) { dirs[3 * k] = t.dirs[k].x; dirs[3 * k + 1] = t.dirs[k].y; dirs[3 * k + 2] = t.dirs[k].z; }
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

// kd: the interior nodes a step calls Kd (rbspkd's axis nodes); maxTodo: the largest todoPos the ray reached (the entries it held at once)
struct WalkCount { uint64_t nodes = 0, interior = 0, leaves = 0, kd = 0; uint32_t maxTodo = 0, maxTodoDot = 0; };      // maxTodoDot: the same over the pushes made at interior nodes the step does not call Kd

// A baked scene (no instances), its BVH (for the ordered numbering and the primitive tests) and a tree walked with Step's
// interior step.  A Step names its node type (NodeT: the two leading words are the 8-byte node's) and supplies
//   Shift(tree)                 the shift of the high bits (nPrims, aboveChild)
//   IsLeaf(tree, node), Kd(tree, node)
//   Interior(tree, node, ray, invDir, &tPlane, &belowFirst)
// and, where the split planes are listed (SceneSplits), Axis(tree, node).
template <class Step> struct SceneRef {
    typedef typename Step::NodeT NodeT;
    struct ToDo { const NodeT *node; Float tMin, tMax; };

    Scene scene;
    std::vector<BVH> objectBvh;
    BVH bvh;                       // primOrder: ordered -> creation number (the device numbering), and the primitive tests
    std::vector<uint32_t> toOrdered;
    TreeT<NodeT> tree;
    Step step;
    mutable std::vector<uint32_t> maxTodoDot;   // and WalkCount::maxTodoDot
    mutable std::vector<uint32_t> maxTodo;      // per ray of the last IntersectRays / OccludedRays: WalkCount::maxTodo

    // KdTreeAccel::Intersect (accelerators/kdtreeaccel.cpp:381-457), RBSP::Intersect (rbsp.cpp:405-477), RBSPKd::Intersect
    // (rbspKd.cpp:490-565), BSP::Intersect (BSP.cpp)
    bool Intersect(const Ray &ray, SurfaceInteraction *isect, Counters &ctr, WalkCount &wc) const {
        const uint32_t off = step.Shift(tree);
        Float tMin, tMax;
        if (!RootInterval(tree.bounds, ray, &tMin, &tMax)) return false;
        const V3 invDir(1 / ray.d.x, 1 / ray.d.y, 1 / ray.d.z);
        ToDo todo[64];
        uint32_t todoPos = 0;
        bool hit = false;
        const NodeT *node = &tree.nodes[0];
        while (node != nullptr) {
            if (ray.tMax < tMin) break;
            ++wc.nodes;
            if (!step.IsLeaf(tree, node)) {
                ++wc.interior;
                if (step.Kd(tree, node)) ++wc.kd;
                Float tPlane; bool belowFirst;
                step.Interior(tree, node, ray, invDir, &tPlane, &belowFirst);
                const NodeT *first, *second;
                if (belowFirst) { first = node + 1; second = &tree.nodes[node->aboveChild >> off]; }
                else { first = &tree.nodes[node->aboveChild >> off]; second = node + 1; }
                if (tPlane > tMax || tPlane <= 0) node = first;
                else if (tPlane < tMin) node = second;
                else {
                    todo[todoPos].node = second; todo[todoPos].tMin = tPlane; todo[todoPos].tMax = tMax; ++todoPos;
                    wc.maxTodo = std::max(wc.maxTodo, todoPos);
                    if (!step.Kd(tree, node)) wc.maxTodoDot = std::max(wc.maxTodoDot, todoPos);
                    node = first; tMax = tPlane;
                }
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
    // KdTreeAccel::IntersectP (:459-521), RBSP::IntersectP (:479-547), RBSPKd::IntersectP (:567-638), BSP::IntersectP: the leaf
    // test comes first
    bool IntersectP(const Ray &ray, Counters &ctr, WalkCount &wc) const {
        const uint32_t off = step.Shift(tree);
        Float tMin, tMax;
        if (!RootInterval(tree.bounds, ray, &tMin, &tMax)) return false;
        const V3 invDir(1 / ray.d.x, 1 / ray.d.y, 1 / ray.d.z);
        ToDo todo[64];
        uint32_t todoPos = 0;
        const NodeT *node = &tree.nodes[0];
        while (node != nullptr) {
            ++wc.nodes;
            if (step.IsLeaf(tree, node)) {
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
                if (step.Kd(tree, node)) ++wc.kd;
                Float tPlane; bool belowFirst;
                step.Interior(tree, node, ray, invDir, &tPlane, &belowFirst);
                const NodeT *first, *second;
                if (belowFirst) { first = node + 1; second = &tree.nodes[node->aboveChild >> off]; }
                else { first = &tree.nodes[node->aboveChild >> off]; second = node + 1; }
                if (tPlane > tMax || tPlane <= 0) node = first;
                else if (tPlane < tMin) node = second;
                else {
                    todo[todoPos].node = second; todo[todoPos].tMin = tPlane; todo[todoPos].tMax = tMax; ++todoPos;
                    wc.maxTodo = std::max(wc.maxTodo, todoPos);
                    if (!step.Kd(tree, node)) wc.maxTodoDot = std::max(wc.maxTodoDot, todoPos);
                    node = first; tMax = tPlane;
                }
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

// the scene, its BVH, the ordered numbering and the world bounds as the tree's; null (g_err) for an unreadable or instanced scene
template <class Step> SceneRef<Step> *LoadSceneRef(const char *path) {
    SceneRef<Step> *r = new SceneRef<Step>();
    std::string err;
    if (!LoadScene(path, &r->scene, &err)) { g_err = err; delete r; return nullptr; }
    if (!r->scene.instances.empty()) { g_err = "instanced scene"; delete r; return nullptr; }
    r->bvh.Build(&r->scene, &r->scene.prims, &r->objectBvh, 0);
    const size_t n = r->scene.prims.size();
    r->toOrdered.resize(n);
    for (size_t i = 0; i < n; ++i) r->toOrdered[r->bvh.primOrder[i]] = (uint32_t)i;
    r->tree.bounds = B3();
    for (size_t i = 0; i < n; ++i) r->tree.bounds = Union(r->tree.bounds, r->bvh.PrimWorldBound((uint32_t)i));
    return r;
}

template <class Step> void SceneSetTree(SceneRef<Step> *r, size_t nNodes, const void *nodes, size_t nIdx, const uint32_t *idx) {
    r->tree.nodes.resize(nNodes);
    memcpy(r->tree.nodes.data(), nodes, nNodes * sizeof(typename Step::NodeT));
    r->tree.primitiveIndices.assign(idx, idx + nIdx);
}

// sizes[0..1] = nodes, primitiveIndices entries; the arrays where nodes is given
template <class Step> void SceneTree(const SceneRef<Step> *r, uint32_t sizes[2], void *nodes, uint32_t *idx) {
    sizes[0] = (uint32_t)r->tree.nodes.size(); sizes[1] = (uint32_t)r->tree.primitiveIndices.size();
    if (nodes) CopyTree(r->tree, nodes, idx, nullptr);
}

// the scene's triangles in creation order (9 floats each; other primitives are skipped); returns how many
template <class Step> size_t SceneTriangles(const SceneRef<Step> *r, float *p9) {
    size_t k = 0;
    for (const Prim &p : r->Prims())
        if (p.tri) { for (int v = 0; v < 3; ++v) { p9[9 * k + 3 * v] = p.p[v].x; p9[9 * k + 3 * v + 1] = p.p[v].y; p9[9 * k + 3 * v + 2] = p.p[v].z; } ++k; }
    return k;
}

// the split planes of the scene's tree (axis or direction, position) of the first `cap` interior nodes
template <class Step> size_t SceneSplits(const SceneRef<Step> *r, int32_t *axis, float *pos, size_t cap) {
    size_t k = 0;
    for (const typename Step::NodeT &nd : r->tree.nodes)
        if (!r->step.IsLeaf(r->tree, &nd) && k < cap) { axis[k] = (int32_t)r->step.Axis(r->tree, &nd); pos[k] = nd.split; ++k; }
    return k;
}

// counters per ray, W = 4 or 5 columns: nodes (nbNodeTraversals), interior nodes (kdTreeNodeTraversals / bspTreeNodeTraversals),
// triangle tests, sphere tests and, in a fifth column, the interior nodes the step calls Kd
template <class Step> void IntersectRays(const SceneRef<Step> *r, size_t n, const float *o, const float *d, const float *tmax, float *tOut,
                                         int32_t *primOut, float *bary, uint64_t *counters, int W) {
    r->maxTodo.assign(n, 0u); r->maxTodoDot.assign(n, 0u);
    for (size_t i = 0; i < n; ++i) {
        Ray ray(V3(o[3 * i], o[3 * i + 1], o[3 * i + 2]), V3(d[3 * i], d[3 * i + 1], d[3 * i + 2]), tmax[i]);
        SurfaceInteraction si; Counters c; WalkCount wc;
        const bool hit = r->Intersect(ray, &si, c, wc);
        r->maxTodo[i] = wc.maxTodo; r->maxTodoDot[i] = wc.maxTodoDot;
        tOut[i] = ray.tMax; primOut[i] = hit ? si.ordered : -1;
        bary[3 * i] = hit ? si.b0 : 0.f; bary[3 * i + 1] = hit ? si.b1 : 0.f; bary[3 * i + 2] = hit ? si.b2 : 0.f;
        counters[W * i] = wc.nodes; counters[W * i + 1] = wc.interior; counters[W * i + 2] = c.triTests; counters[W * i + 3] = c.sphereTests;
        if (W == 5) counters[W * i + 4] = wc.kd;
    }
}
template <class Step> void OccludedRays(const SceneRef<Step> *r, size_t n, const float *o, const float *d, const float *tmax, uint8_t *occ,
                                        uint64_t *counters, int W) {
    r->maxTodo.assign(n, 0u); r->maxTodoDot.assign(n, 0u);
    for (size_t i = 0; i < n; ++i) {
        Ray ray(V3(o[3 * i], o[3 * i + 1], o[3 * i + 2]), V3(d[3 * i], d[3 * i + 1], d[3 * i + 2]), tmax[i]);
        Counters c; WalkCount wc;
        occ[i] = r->IntersectP(ray, c, wc) ? 1 : 0;
        r->maxTodo[i] = wc.maxTodo; r->maxTodoDot[i] = wc.maxTodoDot;
        counters[W * i] = wc.nodes; counters[W * i + 1] = wc.interior; counters[W * i + 2] = c.triTestsP; counters[W * i + 3] = c.sphereTestsP;
        if (W == 5) counters[W * i + 4] = wc.kd;
    }
}
// the optional per-ray output of the two walks: the largest todoPos of each ray of the last IntersectRays / OccludedRays call;
// returns how many
template <class Step> size_t SceneMaxTodo(const SceneRef<Step> *r, uint32_t *out) {
    if (out) std::copy(r->maxTodo.begin(), r->maxTodo.end(), out);
    return r->maxTodo.size();
}
template <class Step> size_t SceneMaxTodoDot(const SceneRef<Step> *r, uint32_t *out) {
    if (out) std::copy(r->maxTodoDot.begin(), r->maxTodoDot.end(), out);
    return r->maxTodoDot.size();
}

}  // namespace
