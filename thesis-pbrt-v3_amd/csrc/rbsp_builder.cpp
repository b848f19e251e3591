// hprt — RBSP::buildTree (accelerators/rbsp.cpp:181-403) and RBSPKd::buildTree (accelerators/rbspKd.cpp:194-488,
// RbspParams::kdAware) with KDOPCut / KDOPSurfaceArea (accelerators/kDOPMesh.h), restated operation for operation.  Every float
// operation is one IEEE rounding in the reference's order (built with -ffp-contract=off).
//
// The one liberty: the candidates of a node may be costed on several threads.  Each candidate's cost is a pure function of the
// node's k-DOP and the candidate, and the reduction keeps the first minimum in (direction, edge) order — what the reference's
// strict `cost < bestCost` scan keeps (for RBSPKd, each of its two minima) — so the tree does not depend on the thread count.
// The winner's two halves are then cut and measured once more, exactly as the scan left them.
#include "rbsp_builder.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <thread>

namespace hprt {
namespace {

struct P3 { float x, y, z; };
inline bool Same(const P3 &a, const P3 &b) { return a.x == b.x && a.y == b.y && a.z == b.z; }   // Point3::operator==
inline float Dot(const float *d, const P3 &p) { return d[0] * p.x + d[1] * p.y + d[2] * p.z; }   // Dot(Vector3f, Point3f)
inline float fmin_std(float a, float b) { return (b < a) ? b : a; }   // std::min
inline float fmax_std(float a, float b) { return (a < b) ? b : a; }   // std::max

struct KEdge { P3 v1, v2; uint32_t f1, f2; };                       // KDOPEdge
using Mesh = std::vector<KEdge>;                                    // KDOPMesh::edges

// per-thread scratch of KDOPCut / KDOPSurfaceArea (the reference allocates these per call)
struct Scratch {
    std::vector<std::vector<P3>> faceVertices;
    std::vector<KEdge> coincident;
    std::vector<std::vector<uint32_t>> faces;
    std::vector<uint8_t> used;
    Mesh left, right;
    void reset(uint32_t M) {
        faceVertices.resize(2 * M); for (auto &f : faceVertices) f.clear();
        faces.resize(2 * M); for (auto &f : faces) f.clear();
        coincident.clear();
    }
};

// KDOPCutHelper: add a vertex to a face's list unless it is there already
inline void AddVertex(std::vector<P3> &pts, const P3 &p) {
    for (const P3 &q : pts) if (Same(q, p)) return;
    pts.push_back(p);
}
// KDOPMeshBase::addEdgeIfNeeded: an edge with the same end points in either orientation is not added again
inline void AddEdgeIfNeeded(Mesh &m, const KEdge &e) {
    for (const KEdge &f : m)
        if ((Same(f.v1, e.v2) && Same(f.v2, e.v1)) || (Same(f.v1, e.v1) && Same(f.v2, e.v2))) return;
    m.push_back(e);
}

// KDOPCutAddEdge (kDOPMesh.h): t1 <= t2 are the projections of the (oriented) edge's end points
inline void CutAddEdge(Scratch &s, const KEdge &edge, float t, float t1, float t2) {
    if (t1 < t && t2 < t) s.left.push_back(edge);
    else if (t1 > t && t2 > t) s.right.push_back(edge);
    else if (t1 < t && t == t2) {
        s.left.push_back(edge);
        AddVertex(s.faceVertices[edge.f1], edge.v2); AddVertex(s.faceVertices[edge.f2], edge.v2);
    } else if (t1 == t && t < t2) {
        s.right.push_back(edge);
        AddVertex(s.faceVertices[edge.f1], edge.v1); AddVertex(s.faceVertices[edge.f2], edge.v1);
    } else if (t1 < t && t < t2) {
        const float dx = edge.v2.x - edge.v1.x, dy = edge.v2.y - edge.v1.y, dz = edge.v2.z - edge.v1.z;
        const float tAlongEdge = (-(t1 - t)) / (t2 - t1);
        const P3 vs{edge.v1.x + tAlongEdge * dx, edge.v1.y + tAlongEdge * dy, edge.v1.z + tAlongEdge * dz};
        s.left.push_back(KEdge{edge.v1, vs, edge.f1, edge.f2});
        s.right.push_back(KEdge{vs, edge.v2, edge.f1, edge.f2});
        AddVertex(s.faceVertices[edge.f1], vs); AddVertex(s.faceVertices[edge.f2], vs);
    } else if (t1 == t && t == t2) s.coincident.push_back(edge);
}

// KDOPCut (kDOPMesh.h): the halves below (s.left) and above (s.right) the plane Dot(direction, p) = t
void Cut(const Mesh &edges, uint32_t M, float t, const float *direction, uint32_t directionId, Scratch &s) {
    s.reset(M);
    s.left.clear(); s.right.clear();
    for (const KEdge &edge : edges) {
        const float t1 = Dot(direction, edge.v1), t2 = Dot(direction, edge.v2);
        if (t1 > t2) CutAddEdge(s, KEdge{edge.v2, edge.v1, edge.f1, edge.f2}, t, t2, t1);
        else CutAddEdge(s, edge, t, t1, t2);
    }
    for (const KEdge &edge : s.coincident) {
        // the first left edge sharing one of its faces decides which half keeps which face (the loop ends at the first match)
        for (size_t k = 0; k < s.left.size(); ++k) {
            const KEdge le = s.left[k];
            if (le.f1 == edge.f1 || le.f2 == edge.f1) {
                s.left.push_back(KEdge{edge.v1, edge.v2, edge.f1, 2 * directionId});
                s.right.push_back(KEdge{edge.v1, edge.v2, edge.f2, 2 * directionId + 1});
                break;
            } else if (le.f1 == edge.f2 || le.f2 == edge.f2) {
                s.left.push_back(KEdge{edge.v1, edge.v2, edge.f2, 2 * directionId});
                s.right.push_back(KEdge{edge.v1, edge.v2, edge.f1, 2 * directionId + 1});
                break;
            }
        }
    }
    for (uint32_t i = 0; i < 2 * M; ++i) {
        const std::vector<P3> &fv = s.faceVertices[i];
        if (fv.size() == 2) {
            AddEdgeIfNeeded(s.left, KEdge{fv[0], fv[1], i, 2 * directionId});
            AddEdgeIfNeeded(s.right, KEdge{fv[0], fv[1], i, 2 * directionId + 1});
        }
    }
}

// KDOPSurfaceArea (kDOPMesh.h).  It MUTATES the mesh: chaining a face swaps v1 / v2 of the edges it walks into, and the
// reference stores the meshes after this call, so the orientation is inherited by later cuts.  Cross in double, rounded to float.
float SurfaceArea(Mesh &edges, const float *dirs, uint32_t M, Scratch &s) {
    s.faces.resize(2 * M);
    for (uint32_t i = 0; i < 2 * M; ++i) s.faces[i].clear();
    for (uint32_t k = 0; k < (uint32_t)edges.size(); ++k) { s.faces[edges[k].f1].push_back(k); s.faces[edges[k].f2].push_back(k); }
    float SA = 0;
    for (uint32_t i = 0; i < 2 * M; ++i) {
        float fx = 0, fy = 0, fz = 0;
        const std::vector<uint32_t> &face = s.faces[i];
        if (!face.empty()) {
            s.used.assign(face.size(), 0);
            uint32_t edgeId = 0;
            do {
                if (s.used[edgeId]) break;
                s.used[edgeId] = 1;
                const KEdge &cur = edges[face[edgeId]];
                const double v1x = cur.v1.x, v1y = cur.v1.y, v1z = cur.v1.z, v2x = cur.v2.x, v2y = cur.v2.y, v2z = cur.v2.z;
                fx += (float)((v1y * v2z) - (v1z * v2y));
                fy += (float)((v1z * v2x) - (v1x * v2z));
                fz += (float)((v1x * v2y) - (v1y * v2x));
                for (uint32_t j = 0; j < (uint32_t)face.size(); ++j) {
                    if (j == edgeId) continue;
                    // (cur may be ej itself when an edge lists the same face twice: the swap then moves cur.v2 too, as in the reference)
                    KEdge &ej = edges[face[j]];
                    if (Same(ej.v2, cur.v2)) std::swap(ej.v1, ej.v2);
                    if (Same(ej.v1, cur.v2) && !s.used[j]) { edgeId = j; break; }
                }
            } while (edgeId != 0);
        }
        const float *d = dirs + 3 * (i / 2);
        SA += std::abs(d[0] * fx + d[1] * fy + d[2] * fz);
    }
    return SA / 2.0f;
}

enum class EdgeType : int { Start, End };
struct BoundEdge { float t; uint32_t primNum; EdgeType type; };     // accelerators/genericBSP.h:47-58
struct Range { float min, max; };                                   // Bounds<Float>
struct BuildNode {                                                  // RBSPBuildNode, accelerators/RBSPShared.h:11-27
    uint32_t depth, nPrimitives, badRefines;
    std::vector<Range> nodeBounds;
    Mesh mesh; float meshArea;
    size_t primNums; uint32_t parentNum;                            // primNums: offset into `prims`
};
struct Cand { uint32_t d, i, nBelow, nAbove; float t; };

// Log2Int(int64_t) (core/pbrt.h:345-362): 63 - clz
inline int Log2Int64(uint64_t v) { return v ? 63 - __builtin_clzll(v) : -1; }

int ThreadCount(int requested) {
    int n = requested;
    if (n <= 0) {
        const char *e = std::getenv("OMP_NUM_THREADS");
        n = e ? std::atoi(e) : 16;
    }
    return std::max(1, std::min(16, n));
}

// Below this many candidates a node is costed on the calling thread: spawning threads would cost more than it saves.
constexpr size_t kParallelCandidates = 1024;

}  // namespace

bool RbspDirections(uint32_t M, std::vector<float> *out) {
    if (M != 3 && M != 7 && M != 9 && M != 13) return false;
    std::vector<float> &d = *out;
    d.clear();
    auto add = [&](float x, float y, float z) { d.push_back(x); d.push_back(y); d.push_back(z); };
    auto addNormalized = [&](float x, float y, float z) {
        // Normalize(v) = v / v.Length() and Vector3::operator/ multiplies by (Float)1 / f
        const float len = std::sqrt(x * x + y * y + z * z);
        const float inv = (float)1 / len;
        add(x * inv, y * inv, z * inv);
    };
    add(1.f, 0.f, 0.f); add(0.f, 1.f, 0.f); add(0.f, 0.f, 1.f);
    if (M == 7 || M == 13) {
        addNormalized(1.f, 1.f, 1.f); addNormalized(1.f, -1.f, 1.f); addNormalized(1.f, 1.f, -1.f); addNormalized(1.f, -1.f, -1.f);
    }
    if (M == 9 || M == 13) {
        addNormalized(1.f, 1.f, 0.f); addNormalized(1.f, 0.f, 1.f); addNormalized(0.f, 1.f, 1.f);
        addNormalized(1.f, -1.f, 0.f); addNormalized(1.f, 0.f, -1.f); addNormalized(0.f, 1.f, -1.f);
    }
    return true;
}

std::string BuildRbspTree(size_t n, const float *bmin, const float *bmax, const float *tri9, const uint8_t *isTri, const RbspParams &p,
                          RbspTree *out) {
    RbspTree &t = *out;
    t = RbspTree();
    const uint32_t M = (uint32_t)p.nDirections;
    if (p.nDirections <= 0 || !RbspDirections(M, &t.directions))
        return "nbDirections " + std::to_string(p.nDirections) + " is not supported (3, 7, 9 or 13)";
    const float *dirs = t.directions.data();
    const uint32_t off = RbspBitOffset(M);
    // CreateRBSPTreeAccelerator / GenericBSP: the parameters as the reference holds them (uint32_t, Float)
    const uint32_t isectCost = (uint32_t)p.isectCost, traversalCost = (uint32_t)p.travCost, maxPrims = (uint32_t)p.maxPrims;
    const float emptyBonus = p.emptyBonus;
    uint32_t maxDepth = (uint32_t)p.maxDepth;
    if (maxDepth == (uint32_t)-1) maxDepth = (uint32_t)std::round(2 + 1.6f * (float)Log2Int64((uint64_t)n));   // calculateMaxDepth
    t.nPrims = (uint32_t)n; t.M = M; t.maxDepth = maxDepth;
    const int nThreads = ThreadCount(p.threads);

    // bounds = Union of every WorldBound; per-direction root bounds = Union of the primitives' projections (getBounds)
    float lo[3], hi[3];
    for (int k = 0; k < 3; ++k) { lo[k] = std::numeric_limits<float>::max(); hi[k] = std::numeric_limits<float>::lowest(); }
    std::vector<Range> root(M, Range{std::numeric_limits<float>::max(), std::numeric_limits<float>::lowest()});
    std::vector<Range> allPrimBounds((size_t)n * M);
    for (size_t i = 0; i < n; ++i) {
        for (int k = 0; k < 3; ++k) { lo[k] = fmin_std(lo[k], bmin[3 * i + k]); hi[k] = fmax_std(hi[k], bmax[3 * i + k]); }
        for (uint32_t d = 0; d < M; ++d) {
            const float *dir = dirs + 3 * d;
            Range b;
            if (isTri[i]) {     // Triangle::getBounds
                const float *v = tri9 + 9 * i;
                float tt = Dot(dir, P3{v[0], v[1], v[2]});
                float mn = tt, mx = tt;
                for (int c = 1; c < 3; ++c) {
                    tt = Dot(dir, P3{v[3 * c], v[3 * c + 1], v[3 * c + 2]});
                    if (tt > mx) mx = tt;
                    else if (tt < mn) mn = tt;
                }
                b = Range{mn, mx};
            } else {            // Shape::getBounds: the 8 corners of WorldBound (Bounds3::Corner)
                b = Range{std::numeric_limits<float>::max(), std::numeric_limits<float>::lowest()};
                const float *bl = bmin + 3 * i, *bh = bmax + 3 * i;
                for (int c = 0; c < 8; ++c) {
                    const P3 q{(c & 1) ? bh[0] : bl[0], (c & 2) ? bh[1] : bl[1], (c & 4) ? bh[2] : bl[2]};
                    const float proj = Dot(dir, q);
                    if (proj < b.min) b.min = proj;
                    if (proj > b.max) b.max = proj;
                }
            }
            allPrimBounds[i * M + d] = b;
            root[d] = Range{fmin_std(root[d].min, b.min), fmax_std(root[d].max, b.max)};
        }
    }
    for (int k = 0; k < 3; ++k) { t.bounds[k] = lo[k]; t.bounds[3 + k] = hi[k]; }

    // Bounds3::toKDOPMesh (core/geometry.h:1001-1027): the 12 edges of the box with their face ids
    Mesh rootMesh;
    {
        const P3 v1{lo[0], lo[1], lo[2]}, v2{lo[0], lo[1], hi[2]}, v3{lo[0], hi[1], lo[2]}, v4{hi[0], lo[1], lo[2]};
        const P3 v5{lo[0], hi[1], hi[2]}, v6{hi[0], lo[1], hi[2]}, v7{hi[0], hi[1], lo[2]}, v8{hi[0], hi[1], hi[2]};
        rootMesh = {{v1, v2, 1, 3}, {v1, v3, 1, 5}, {v1, v4, 3, 5}, {v2, v5, 1, 4}, {v2, v6, 3, 4}, {v3, v5, 1, 2},
                    {v3, v7, 2, 5}, {v4, v6, 0, 3}, {v4, v7, 0, 5}, {v5, v8, 2, 4}, {v6, v8, 0, 4}, {v7, v8, 0, 2}};
    }
    std::vector<Scratch> scratch((size_t)nThreads);
    const float rootArea = SurfaceArea(rootMesh, dirs, M, scratch[0]);    // evaluated before the mesh is stored

    std::vector<std::vector<BoundEdge>> edges(M);
    for (auto &e : edges) e.resize(2 * n);
    // the reference's primitive buffer: (maxDepth + 1) * N entries, written without a check; here a write past it is an error
    const uint64_t primsCap = ((uint64_t)maxDepth + 1) * (uint64_t)n;
    std::vector<uint32_t> prims(n + 1);
    for (size_t i = 0; i < n; ++i) prims[i] = (uint32_t)i;

    std::vector<RbspNode> &nodes = t.nodes;
    auto initLeaf = [&](const uint32_t *primNums, uint32_t np) {     // RBSPNode::InitLeaf (:163-177)
        RbspNode nd;
        nd.b = M | (np << off);
        if (np == 0) nd.a = 0u;
        else if (np == 1) nd.a = primNums[0];
        else {
            nd.a = (uint32_t)t.primIndices.size();
            for (uint32_t i = 0; i < np; ++i) t.primIndices.push_back(primNums[i]);
        }
        nodes.push_back(nd);
        ++t.leaves;
    };

    std::vector<Cand> cands;
    std::vector<float> costs, costsFixed;       // costsFixed: RBSPKd's traversalCost + C_isect of the oblique candidates
    const float BSP_ALPHA = 0.1;                 // RBSPKd::buildTree's `const Float`
    const uint32_t kdTraversalCost = (uint32_t)p.kdTravCost;
    std::vector<std::thread> pool;
    uint32_t nodeNum = 0;
    std::vector<BuildNode> stack;
    stack.push_back(BuildNode{maxDepth, (uint32_t)n, 0u, root, rootMesh, rootArea, 0, (uint32_t)-1});
    while (!stack.empty()) {
        BuildNode cur = std::move(stack.back());
        stack.pop_back();
        if (cur.parentNum != (uint32_t)-1) nodes[cur.parentNum].b |= (nodeNum << off);      // setAboveChild

        if (cur.nPrimitives <= maxPrims || cur.depth == 0) { initLeaf(&prims[cur.primNums], cur.nPrimitives); ++nodeNum; continue; }

        const float oldCost = (float)isectCost * float(cur.nPrimitives);
        const float invTotalSA = 1 / cur.meshArea;
        // every candidate of every direction, in the reference's scan order
        cands.clear();
        for (uint32_t d = 0; d < M; ++d) {
            BoundEdge *e = edges[d].data();
            const uint32_t *primNums = &prims[cur.primNums];
            for (uint32_t i = 0; i < cur.nPrimitives; ++i) {
                const uint32_t pn = primNums[i];
                const Range &b = allPrimBounds[(size_t)pn * M + d];
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
                if (edgeT > cur.nodeBounds[d].min && edgeT < cur.nodeBounds[d].max) cands.push_back(Cand{d, i, nBelow, nAbove, edgeT});
                if (e[i].type == EdgeType::Start) ++nBelow;
            }
        }
        costs.resize(cands.size());
        if (p.kdAware) costsFixed.resize(cands.size());
        auto costRange = [&](size_t k0, size_t k1, Scratch &s) {
            for (size_t k = k0; k < k1; ++k) {
                const Cand &c = cands[k];
                Cut(cur.mesh, M, c.t, dirs + 3 * c.d, c.d, s);
                const float areaBelow = SurfaceArea(s.left, dirs, M, s);
                const float areaAbove = SurfaceArea(s.right, dirs, M, s);
                const float pBelow = areaBelow * invTotalSA;
                const float pAbove = areaAbove * invTotalSA;
                const float eb = (c.nAbove == 0 || c.nBelow == 0) ? emptyBonus : 0;
                if (!p.kdAware) {
                    costs[k] = (float)traversalCost + (float)isectCost * (1 - eb) * (pBelow * (float)c.nBelow + pAbove * (float)c.nAbove);
                } else if (c.d < 3) {
                    costs[k] = (float)kdTraversalCost + (float)isectCost * (1 - eb) * (pBelow * (float)c.nBelow + pAbove * (float)c.nAbove);
                } else {
                    const float costIntersection = (float)isectCost * (1 - eb) * (pBelow * (float)c.nBelow + pAbove * (float)c.nAbove);
                    costsFixed[k] = (float)traversalCost + costIntersection;
                    costs[k] = BSP_ALPHA * (float)isectCost * (float)(cur.nPrimitives - 1) + (float)kdTraversalCost + costIntersection;
                }
            }
        };
        if (nThreads > 1 && cands.size() >= kParallelCandidates) {
            const size_t chunk = (cands.size() + nThreads - 1) / nThreads;
            pool.clear();
            for (int w = 1; w < nThreads; ++w) {
                const size_t k0 = std::min(cands.size(), w * chunk), k1 = std::min(cands.size(), (w + 1) * chunk);
                pool.emplace_back(costRange, k0, k1, std::ref(scratch[(size_t)w]));
            }
            costRange(0, std::min(cands.size(), chunk), scratch[0]);
            for (auto &th : pool) th.join();
        } else costRange(0, cands.size(), scratch[0]);
        // the reference's scan: strict `<`, so the first minimum in (direction, edge) order
        uint32_t bestD = (uint32_t)-1, bestOffset = (uint32_t)-1;
        float bestCost = std::numeric_limits<float>::infinity();
        for (size_t k = 0; k < cands.size(); ++k)
            if (costs[k] < bestCost) { bestCost = costs[k]; bestD = cands[k].d; bestOffset = cands[k].i; }

        if (p.kdAware) {
            // RBSPKd keeps a second minimum over the oblique candidates (costFixed); the leaf tests need both to fail
            uint32_t bestDFixed = (uint32_t)-1;
            float bestCostFixed = std::numeric_limits<float>::infinity();
            for (size_t k = 0; k < cands.size(); ++k)
                if (cands[k].d >= 3 && costsFixed[k] < bestCostFixed) { bestCostFixed = costsFixed[k]; bestDFixed = cands[k].d; }
            if (bestCost > oldCost && bestCostFixed > oldCost) ++cur.badRefines;
            if ((bestCost > 4 * oldCost && bestCostFixed > 4 * oldCost && cur.nPrimitives < 16) || (bestD == (uint32_t)-1 && bestDFixed == (uint32_t)-1) ||
                cur.badRefines == 3) {
                initLeaf(&prims[cur.primNums], cur.nPrimitives); ++nodeNum; continue;
            }
            // only the fixed minimum beat infinity: the reference classifies by edges[bestD = -1] (rbspKd.cpp:423-432)
            if (bestD == (uint32_t)-1)
                return "every kd-aware candidate cost is infinite or NaN while a fixed-cost oblique split exists: the reference's build is undefined there";
        } else {
            // Create leaf if no good splits were found
            if (bestCost > oldCost) ++cur.badRefines;
            if ((bestCost > 4 * oldCost && cur.nPrimitives < 16) || bestD == (uint32_t)-1 || cur.badRefines == 3) {
                initLeaf(&prims[cur.primNums], cur.nPrimitives); ++nodeNum; continue;
            }
        }

        // the winner's halves, measured (and so reoriented) as the scan left them
        const BoundEdge *e = edges[bestD].data();
        const float tSplit = e[bestOffset].t;
        Scratch &s = scratch[0];
        Cut(cur.mesh, M, tSplit, dirs + 3 * bestD, bestD, s);
        Mesh below = s.left, above = s.right;
        const float areaBelow = SurfaceArea(below, dirs, M, s);
        const float areaAbove = SurfaceArea(above, dirs, M, s);

        // Classify primitives with respect to split: prims1 first, in place, so that child 0's share does not overwrite it
        uint32_t n0 = 0, n1 = 0;
        const size_t prims1 = cur.primNums;
        for (uint32_t i = bestOffset + 1; i < 2 * cur.nPrimitives; ++i)
            if (e[i].type == EdgeType::End) prims[prims1 + n1++] = e[i].primNum;
        const size_t prims0 = prims1 + n1;
        uint32_t nStart = 0;
        for (uint32_t i = 0; i < bestOffset; ++i) nStart += e[i].type == EdgeType::Start;
        if ((uint64_t)prims0 + nStart > primsCap)
            return "the build needs more than the reference's (maxDepth + 1) * N primitive slots; lower \"maxdepth\"";
        if (prims.size() < prims0 + nStart + 1) prims.resize(prims0 + nStart + 1);
        for (uint32_t i = 0; i < bestOffset; ++i)
            if (e[i].type == EdgeType::Start) prims[prims0 + n0++] = e[i].primNum;

        // the children's per-direction bounds: the projections of their k-DOP edges (KDOPEdge::getBounds)
        std::vector<Range> bounds0(M, Range{std::numeric_limits<float>::max(), std::numeric_limits<float>::lowest()}), bounds1 = bounds0;
        for (uint32_t d = 0; d < M; ++d) {
            const float *dir = dirs + 3 * d;
            for (const KEdge &ke : below) {
                const float t1 = Dot(dir, ke.v1), t2 = Dot(dir, ke.v2);
                bounds0[d] = Range{fmin_std(bounds0[d].min, fmin_std(t1, t2)), fmax_std(bounds0[d].max, fmax_std(t1, t2))};
            }
            for (const KEdge &ke : above) {
                const float t1 = Dot(dir, ke.v1), t2 = Dot(dir, ke.v2);
                bounds1[d] = Range{fmin_std(bounds1[d].min, fmin_std(t1, t2)), fmax_std(bounds1[d].max, fmax_std(t1, t2))};
            }
        }
        RbspNode nd;                                   // InitInterior
        std::memcpy(&nd.a, &tSplit, 4);
        nd.b = bestD;
        nodes.push_back(nd);
        stack.push_back(BuildNode{cur.depth - 1, n1, cur.badRefines, std::move(bounds1), std::move(above), areaAbove, prims1, nodeNum});
        stack.push_back(BuildNode{cur.depth - 1, n0, cur.badRefines, std::move(bounds0), std::move(below), areaBelow, prims0, (uint32_t)-1});
        ++nodeNum;
    }
    uint32_t depth = 0;
    (void)CheckRbspTree(t, &depth);
    t.depth = depth;
    return "";
}

void RbspInteriorCounts(const RbspTree &t, uint32_t *kd, uint32_t *bsp) {
    const uint32_t mask = RbspBitMask(t.M);
    uint32_t k = 0, b = 0;
    for (const RbspNode &nd : t.nodes) {
        const uint32_t ax = nd.b & mask;
        if (ax == t.M) continue;
        if (ax < 3) ++k; else ++b;
    }
    *kd = k; *bsp = b;
}

const char *CheckRbspTree(const RbspTree &t, uint32_t *depthOut) {
    const uint32_t M = t.M;
    if (M != 3 && M != 7 && M != 9 && M != 13) return "the tree's direction count is not 3, 7, 9 or 13";
    if (t.directions.size() != 3 * (size_t)M) return "the direction table does not hold M directions";
    return CheckBspNodes(t.nodes, t.primIndices, t.nPrims, M, RbspBitOffset(M), RbspBitMask(M), depthOut);
}

}  // namespace hprt
