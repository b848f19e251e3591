// hprt — the k-DOP meshes of the fork's BSP builders (accelerators/kDOPMesh.h): KDOPEdge, KDOPCut and KDOPSurfaceArea, restated
// operation for operation.  A mesh is its edge list; the directions its faces belong to are passed alongside (face 2 i / 2 i + 1
// lie on direction i): the RBSP builders pass their fixed table (KDOPMesh), the bsppaper builder the list a node's mesh carries
// (KDOPMeshWithDirections, whose cuts may append a direction).  Every float operation is one IEEE rounding in the reference's
// order (built with -ffp-contract=off).  Host only, header-only: rbsp_builder.cpp and bsppaper_builder.cpp include it.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstdint>
#include <utility>
#include <vector>

namespace hprt {
namespace kdop {

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
inline void Cut(const Mesh &edges, uint32_t M, float t, const float *direction, uint32_t directionId, Scratch &s) {
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
inline float SurfaceArea(Mesh &edges, const float *dirs, uint32_t M, Scratch &s) {
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

// Threads that cost a node's candidates: `requested`, or OMP_NUM_THREADS (else 16) when it is 0; at most 16
inline int ThreadCount(int requested) {
    int n = requested;
    if (n <= 0) {
        const char *e = std::getenv("OMP_NUM_THREADS");
        n = e ? std::atoi(e) : 16;
    }
    return std::max(1, std::min(16, n));
}

// Below this many candidates a node is costed on the calling thread: spawning threads would cost more than it saves.
constexpr size_t kParallelCandidates = 1024;

}  // namespace kdop
}  // namespace hprt
