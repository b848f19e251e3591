// hprt — the cost of one RBSP split candidate over fixed-capacity storage: KDOPCut + KDOPSurfaceArea (kdop_mesh.h) and the three
// cost formulas of BuildRbspTree's costRange (rbsp_builder.cpp), restated once as __host__ __device__ code.  No std::vector, no
// allocation, every loop bounded by a capacity.  Every float operation is one IEEE rounding in the order kdop_mesh.h has (both
// compilers build with -ffp-contract=off -fno-fast-math); the Cross terms are evaluated in double and rounded to float.
//
// What the vector code keeps in per-call vectors lives here in caller-supplied storage (Store):
//   left / right   the two half-meshes, at most `cap` <= KDOP_MAX_EDGES edges each, 32 bytes an edge as two 16-byte words;
//   fv             faceVertices: TWO points and a saturating 2-bit count per face (see AddVertex below for why that is enough);
//   flist          SurfaceArea's faces[i], the edge list of the face being chained (at most KDOP_MAX_FACE_EDGES entries);
//   coincident     not stored: a coincident edge is an input edge verbatim (t1 == t == t2, so Cut never reorients it), and the
//                  list is a bit mask over the input edges, walked in input order.
// Element k of an array sits at [k * stride]: stride 1 on the host, the number of lanes in flight on the device, so that a
// wave's accesses to edge e coalesce ([edge][lane]).
// A candidate that would exceed a capacity sets *overflow and reports no cost; it never writes past the storage.  The caller
// re-costs it with the vector code.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define KDOP_HD __host__ __device__ inline
#else
#define KDOP_HD inline
#endif

// Edges per half-mesh.  Measured maximum over the test inputs and killeroo-simple: see DESIGN.md 8i.
#define KDOP_MAX_EDGES 48
#define KDOP_MAX_FACES 26          // 2 M, M <= 13
#define KDOP_MAX_FACE_EDGES 32     // entries of one face's edge list (an edge that lists the face twice counts twice)

namespace hprt {
namespace kdopcost {

struct Edge { float v1[3], v2[3]; uint32_t f1, f2; };            // kdop::KEdge, field for field (32 bytes)
struct Cand { uint32_t d, i, nBelow, nAbove; float t; };          // a candidate of BuildRbspTree's scan
struct Scalars {                                                  // what costRange reads besides the mesh and the candidate
    float invTotalSA, emptyBonus;
    uint32_t isectCost, traversalCost, kdTraversalCost, nPrimitives;
    uint32_t maxEdges;                                            // 0 = KDOP_MAX_EDGES; may only lower it
};
struct Q { uint32_t x, y, z, w; };                                // one 16-byte word of the storage
struct Store {
    Q *left, *right;           // edge e: [2 e] = v1.xyz, v2.x;  [2 e + 1] = v2.yz, f1, f2
    Q *fv;                     // face f: [2 f], [2 f + 1] = its first two vertices (xyz)
    size_t stride;
    uint8_t *flist;            // entry j at [j * fstride]
    size_t fstride;
    uint32_t cap;              // <= KDOP_MAX_EDGES
};
// 16-byte words a lane needs: both halves and the face vertices
constexpr size_t kStoreWords = 4 * (size_t)KDOP_MAX_EDGES + 2 * (size_t)KDOP_MAX_FACES;

static_assert(KDOP_MAX_EDGES <= 128 && KDOP_MAX_EDGES % 16 == 0, "the coincident mask has 128 bits");
static_assert(KDOP_MAX_FACE_EDGES <= 32 && KDOP_MAX_EDGES <= 255, "used mask is 32 bits, list entries are bytes");

KDOP_HD uint32_t FBits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
KDOP_HD float BitsF(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }
KDOP_HD bool Same(const float *a, const float *b) { return a[0] == b[0] && a[1] == b[1] && a[2] == b[2]; }   // Point3::operator==
KDOP_HD float Dot(const float *d, const float *p) { return d[0] * p[0] + d[1] * p[1] + d[2] * p[2]; }

KDOP_HD Edge LoadEdge(const Q *base, size_t stride, uint32_t e) {
    const Q a = base[(size_t)(2 * e) * stride], b = base[(size_t)(2 * e + 1) * stride];
    Edge r;
    r.v1[0] = BitsF(a.x); r.v1[1] = BitsF(a.y); r.v1[2] = BitsF(a.z); r.v2[0] = BitsF(a.w);
    r.v2[1] = BitsF(b.x); r.v2[2] = BitsF(b.y); r.f1 = b.z; r.f2 = b.w;
    return r;
}
KDOP_HD void StoreEdge(Q *base, size_t stride, uint32_t e, const Edge &k) {
    base[(size_t)(2 * e) * stride] = Q{FBits(k.v1[0]), FBits(k.v1[1]), FBits(k.v1[2]), FBits(k.v2[0])};
    base[(size_t)(2 * e + 1) * stride] = Q{FBits(k.v2[1]), FBits(k.v2[2]), k.f1, k.f2};
}
KDOP_HD Edge MakeEdge(const float *v1, const float *v2, uint32_t f1, uint32_t f2) {
    Edge r;
    for (int c = 0; c < 3; ++c) { r.v1[c] = v1[c]; r.v2[c] = v2[c]; }
    r.f1 = f1; r.f2 = f2;
    return r;
}

// One candidate's working state
struct Work {
    Store st;
    uint32_t nLeft, nRight;
    uint64_t fvCount;          // 2 bits a face: 0, 1, 2 vertices, 3 = more than two
    uint64_t coin0, coin1;     // input edges that lie in the plane
    bool overflow;
};

KDOP_HD void Push(Work &w, bool right, const Edge &e) {
    uint32_t &n = right ? w.nRight : w.nLeft;
    if (n >= w.st.cap) { w.overflow = true; return; }
    StoreEdge(right ? w.st.right : w.st.left, w.st.stride, n, e);
    ++n;
}

// KDOPCutHelper.  The vector code keeps every distinct vertex of a face, but Cut reads a face's list only as "is its size
// exactly 2, and which two".  A list never shrinks, so once a third distinct vertex has arrived the size is never 2 again and
// nothing of the list is read: the count saturates at 3 and later vertices are dropped.  Up to that point every vertex of the
// list is stored, so the duplicate test is the vector code's.
KDOP_HD void AddVertex(Work &w, uint32_t face, const float *p) {
    const uint32_t cnt = (uint32_t)(w.fvCount >> (2 * face)) & 3u;
    if (cnt == 3) return;
    for (uint32_t k = 0; k < cnt; ++k) {
        const Q q = w.st.fv[(size_t)(2 * face + k) * w.st.stride];
        const float v[3] = {BitsF(q.x), BitsF(q.y), BitsF(q.z)};
        if (Same(v, p)) return;
    }
    if (cnt < 2) w.st.fv[(size_t)(2 * face + cnt) * w.st.stride] = Q{FBits(p[0]), FBits(p[1]), FBits(p[2]), 0u};
    w.fvCount += (uint64_t)1 << (2 * face);
}

// KDOPMeshBase::addEdgeIfNeeded
KDOP_HD void AddEdgeIfNeeded(Work &w, bool right, const Edge &e) {
    const Q *base = right ? w.st.right : w.st.left;
    const uint32_t n = right ? w.nRight : w.nLeft;
    for (uint32_t k = 0; k < n; ++k) {
        const Edge f = LoadEdge(base, w.st.stride, k);
        if ((Same(f.v1, e.v2) && Same(f.v2, e.v1)) || (Same(f.v1, e.v1) && Same(f.v2, e.v2))) return;
    }
    Push(w, right, e);
}

// KDOPCutAddEdge: t1 <= t2 are the projections of the (oriented) edge's end points; k is the edge's place in the input mesh
KDOP_HD void CutAddEdge(Work &w, const Edge &edge, uint32_t k, float t, float t1, float t2) {
    if (t1 < t && t2 < t) Push(w, false, edge);
    else if (t1 > t && t2 > t) Push(w, true, edge);
    else if (t1 < t && t == t2) {
        Push(w, false, edge);
        AddVertex(w, edge.f1, edge.v2); AddVertex(w, edge.f2, edge.v2);
    } else if (t1 == t && t < t2) {
        Push(w, true, edge);
        AddVertex(w, edge.f1, edge.v1); AddVertex(w, edge.f2, edge.v1);
    } else if (t1 < t && t < t2) {
        const float dx = edge.v2[0] - edge.v1[0], dy = edge.v2[1] - edge.v1[1], dz = edge.v2[2] - edge.v1[2];
        const float tAlongEdge = (-(t1 - t)) / (t2 - t1);
        const float vs[3] = {edge.v1[0] + tAlongEdge * dx, edge.v1[1] + tAlongEdge * dy, edge.v1[2] + tAlongEdge * dz};
        Push(w, false, MakeEdge(edge.v1, vs, edge.f1, edge.f2));
        Push(w, true, MakeEdge(vs, edge.v2, edge.f1, edge.f2));
        AddVertex(w, edge.f1, vs); AddVertex(w, edge.f2, vs);
    } else if (t1 == t && t == t2) {
        if (k < 64) w.coin0 |= (uint64_t)1 << k; else w.coin1 |= (uint64_t)1 << (k - 64);
    }
}

// KDOPCut: the halves below (left) and above (right) the plane Dot(direction, p) = t.  mesh: nE <= cap input edges.
KDOP_HD void Cut(Work &w, const Edge *mesh, uint32_t nE, uint32_t M, float t, const float *direction, uint32_t directionId) {
    w.nLeft = w.nRight = 0; w.fvCount = 0; w.coin0 = w.coin1 = 0;
    for (uint32_t k = 0; k < nE; ++k) {
        const Edge edge = mesh[k];
        const float t1 = Dot(direction, edge.v1), t2 = Dot(direction, edge.v2);
        if (t1 > t2) CutAddEdge(w, MakeEdge(edge.v2, edge.v1, edge.f1, edge.f2), k, t, t2, t1);
        else CutAddEdge(w, edge, k, t, t1, t2);
        if (w.overflow) return;
    }
    for (uint32_t k = 0; k < nE; ++k) {
        if (!(((k < 64 ? w.coin0 >> k : w.coin1 >> (k - 64))) & 1u)) continue;
        const Edge edge = mesh[k];
        // the first left edge sharing one of its faces decides which half keeps which face (the loop ends at the first match)
        const uint32_t nl = w.nLeft;
        for (uint32_t j = 0; j < nl; ++j) {
            const Q b = w.st.left[(size_t)(2 * j + 1) * w.st.stride];
            const uint32_t lf1 = b.z, lf2 = b.w;
            if (lf1 == edge.f1 || lf2 == edge.f1) {
                Push(w, false, MakeEdge(edge.v1, edge.v2, edge.f1, 2 * directionId));
                Push(w, true, MakeEdge(edge.v1, edge.v2, edge.f2, 2 * directionId + 1));
                break;
            } else if (lf1 == edge.f2 || lf2 == edge.f2) {
                Push(w, false, MakeEdge(edge.v1, edge.v2, edge.f2, 2 * directionId));
                Push(w, true, MakeEdge(edge.v1, edge.v2, edge.f1, 2 * directionId + 1));
                break;
            }
        }
        if (w.overflow) return;
    }
    for (uint32_t i = 0; i < 2 * M; ++i) {
        if (((uint32_t)(w.fvCount >> (2 * i)) & 3u) != 2u) continue;
        const Q q0 = w.st.fv[(size_t)(2 * i) * w.st.stride], q1 = w.st.fv[(size_t)(2 * i + 1) * w.st.stride];
        const float a[3] = {BitsF(q0.x), BitsF(q0.y), BitsF(q0.z)}, b[3] = {BitsF(q1.x), BitsF(q1.y), BitsF(q1.z)};
        AddEdgeIfNeeded(w, false, MakeEdge(a, b, i, 2 * directionId));
        AddEdgeIfNeeded(w, true, MakeEdge(a, b, i, 2 * directionId + 1));
        if (w.overflow) return;
    }
}

// KDOPSurfaceArea over one half.  It reorients the edges it chains, in the storage, as the vector code does in its mesh; each
// half's chain order depends on its own swaps only.  faces[i] is rebuilt per face by a scan of the half (an edge that lists face
// i twice enters twice, at neighbouring places, as in the vector code); `used` is a mask over the list's places.
KDOP_HD float SurfaceArea(Work &w, bool right, const float *dirs, uint32_t M) {
    Q *base = right ? w.st.right : w.st.left;
    const uint32_t n = right ? w.nRight : w.nLeft;
    const size_t S = w.st.stride, FS = w.st.fstride;
    uint8_t *list = w.st.flist;
    float SA = 0;
    for (uint32_t i = 0; i < 2 * M; ++i) {
        float fx = 0, fy = 0, fz = 0;
        uint32_t m = 0;
        for (uint32_t k = 0; k < n; ++k) {
            const Q b = base[(size_t)(2 * k + 1) * S];
            if (b.z == i) { if (m >= KDOP_MAX_FACE_EDGES) { w.overflow = true; return 0; } list[m++ * FS] = (uint8_t)k; }
            if (b.w == i) { if (m >= KDOP_MAX_FACE_EDGES) { w.overflow = true; return 0; } list[m++ * FS] = (uint8_t)k; }
        }
        if (m != 0) {
            uint32_t used = 0, edgeId = 0;
            // every pass marks a new place, so at most m passes; the bound is the list's capacity
            for (uint32_t pass = 0; pass <= KDOP_MAX_FACE_EDGES; ++pass) {
                if ((used >> edgeId) & 1u) break;
                used |= 1u << edgeId;
                const uint32_t kc = list[edgeId * FS];
                Edge cur = LoadEdge(base, S, kc);
                const double v1x = cur.v1[0], v1y = cur.v1[1], v1z = cur.v1[2], v2x = cur.v2[0], v2y = cur.v2[1], v2z = cur.v2[2];
                fx += (float)((v1y * v2z) - (v1z * v2y));
                fy += (float)((v1z * v2x) - (v1x * v2z));
                fz += (float)((v1x * v2y) - (v1y * v2x));
                for (uint32_t j = 0; j < m; ++j) {
                    if (j == edgeId) continue;
                    const uint32_t kj = list[j * FS];
                    Edge ej = LoadEdge(base, S, kj);
                    if (Same(ej.v2, cur.v2)) {
                        for (int c = 0; c < 3; ++c) { const float tmp = ej.v1[c]; ej.v1[c] = ej.v2[c]; ej.v2[c] = tmp; }
                        StoreEdge(base, S, kj, ej);
                        if (kj == kc) cur = ej;      // the edge lists this face twice: the swap moved cur.v2 too
                    }
                    if (Same(ej.v1, cur.v2) && !((used >> j) & 1u)) { edgeId = j; break; }
                }
                if (edgeId == 0) break;
            }
        }
        const float *d = dirs + 3 * (i / 2);
        const float s = d[0] * fx + d[1] * fy + d[2] * fz;
        SA += BitsF(FBits(s) & 0x7fffffffu);         // std::abs(float): clears the sign bit
    }
    return SA / 2.0f;
}

// One candidate of costRange.  mesh: the node's k-DOP (nE <= st.cap); dirs: the 3 M direction table.
KDOP_HD void CostCandidate(const Edge *mesh, uint32_t nE, const float *dirs, uint32_t M, bool kdAware, const Scalars &sc, const Cand &c,
                           const Store &st, float *cost, float *costFixed, uint8_t *overflow) {
    Work w;
    w.st = st; w.overflow = false;
    *cost = 0; *costFixed = 0;
    Cut(w, mesh, nE, M, c.t, dirs + 3 * c.d, c.d);
    float areaBelow = 0, areaAbove = 0;
    if (!w.overflow) areaBelow = SurfaceArea(w, false, dirs, M);
    if (!w.overflow) areaAbove = SurfaceArea(w, true, dirs, M);
    if (w.overflow) { *overflow = 1; return; }
    *overflow = 0;
    const float pBelow = areaBelow * sc.invTotalSA;
    const float pAbove = areaAbove * sc.invTotalSA;
    const float eb = (c.nAbove == 0 || c.nBelow == 0) ? sc.emptyBonus : 0;
    const float BSP_ALPHA = 0.1;
    if (!kdAware) {
        *cost = (float)sc.traversalCost + (float)sc.isectCost * (1 - eb) * (pBelow * (float)c.nBelow + pAbove * (float)c.nAbove);
    } else if (c.d < 3) {
        *cost = (float)sc.kdTraversalCost + (float)sc.isectCost * (1 - eb) * (pBelow * (float)c.nBelow + pAbove * (float)c.nAbove);
    } else {
        const float costIntersection = (float)sc.isectCost * (1 - eb) * (pBelow * (float)c.nBelow + pAbove * (float)c.nAbove);
        *costFixed = (float)sc.traversalCost + costIntersection;
        *cost = BSP_ALPHA * (float)sc.isectCost * (float)(sc.nPrimitives - 1) + (float)sc.kdTraversalCost + costIntersection;
    }
}

}  // namespace kdopcost
}  // namespace hprt
