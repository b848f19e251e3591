// hprt — the cost of one general BSP split candidate over fixed-capacity storage: one candidate of BuildBspPaperTree's costRange
// (bsppaper_builder.cpp) restated once as __host__ __device__ code, in the style of kdop_cost.h, whose edge records and 16-byte
// words it reuses.  The extent test of a plane candidate, DirectionId, KDOPMeshWithDirections::cut + the two KDOPSurfaceArea
// calls over the child's directions (bsp_build.h: CutMeasure), NodeBvh::count for a plane candidate and the three cost formulas.
// No std::vector, no allocation, every loop bounded by a capacity.  Every float operation is one IEEE rounding in the vector
// code's order (both compilers build with -ffp-contract=off -fno-fast-math); the Cross terms are evaluated in double and rounded.
//
// Faces.  A general node's direction list grows along the path (3 + up to one per ancestor), but its mesh touches few of them.
// The caller compacts the node once (CompactNode, host): cdir[] lists, ascending, the directions that own a face of the mesh,
// and the mesh's face ids become 2 rank + side.  A candidate's direction either is one of cdir[] or enters it at its place p (a
// new direction at the end with the candidate's axis, one of the node's that owns no face in its order with its own vector), and
// the faces from 2 p on then move up by two as the edges are read: the child's compact table is never stored.  A face that no
// edge lists adds +0 to an area and offers no two-vertex edge to the cut, so leaving it out changes no bit, and the compaction
// keeps the order of the faces, which is the order the vector code adds their areas in.
//
// Storage (Store), element k of an array at [k * stride] as in kdop_cost.h:
//   left / right   the two half-meshes, at most capEdges <= BSP_MAX_EDGES edges each, two 16-byte words an edge;
//   fv             faceVertices: two points per compact face of the child; the saturating count (0, 1, 2, 3 = more) sits in the
//                  fourth word of the first point, so the number of faces is bounded by the storage alone;
//   flist          the edge list of the face being chained (at most capFaceEdges <= BSP_MAX_FACE_EDGES entries);
//   stack          NodeBvh::count's stack of BVH node numbers (at most capStack <= BSP_MAX_STACK entries);
//   coincident     a 128-bit mask over the input edges, as in kdop_cost.h.
// A candidate that would exceed a capacity (or meets a BVH record that points outside the arrays) sets *overflow, writes nothing
// past the storage and reports no cost and no counts; the caller costs it again with the vector code.
#pragma once
#include <cstddef>
#include <cstdint>
#include "kdop_cost.h"

// Measured maxima over the test inputs and killeroo-simple: DESIGN.md 8n.
#ifndef BSP_MAX_EDGES
#define BSP_MAX_EDGES 64           // edges per half-mesh, and of a node's own mesh
#endif
#ifndef BSP_MAX_FACES
#define BSP_MAX_FACES 48          // compact faces of the child: 2 (directions that own a face + the candidate's)
#endif
#ifndef BSP_MAX_FACE_EDGES
#define BSP_MAX_FACE_EDGES 32      // entries of one face's edge list
#endif
#ifndef BSP_MAX_STACK
#define BSP_MAX_STACK 32          // BVH stack entries
#endif
#define BSP_MAX_DIRS 72            // a node's own direction list: 3 + one per level of the walks' 64-entry todo lists, rounded up
#ifndef BSP_NOTE_MAX
#define BSP_NOTE_MAX(which, value) ((void)0)      // (the capacity measurement defines it)
#endif

namespace hprt {
namespace bspcost {

using kdopcost::Edge;
using kdopcost::Q;
using kdopcost::FBits;
using kdopcost::BitsF;
using kdopcost::Same;
using kdopcost::Dot;
using kdopcost::LoadEdge;
using kdopcost::StoreEdge;
using kdopcost::MakeEdge;

struct Cand { uint32_t k, i, nBelow, nAbove; float t, axis[3]; };      // the builder's candidate: k < 3 axis k's edge i, k == 33 a plane
// One node of the BVH over the build node's primitives, as NodeBvh::side reads it: the centre and half the diagonal's length
// (computed on the host with side()'s own operations), LinearBVHNode's offset and (nPrimitives << 2) | axis
struct BvhRec { float c[3], maxDiff; int32_t offset; uint32_t countAxis, pad0, pad1; };
struct Scalars {
    float invTotalSA, emptyBonus;
    uint32_t isectCost, traversalCost, kdTraversalCost, nPrimitives;
    uint32_t maxEdges, maxFaces, maxFaceEdges, maxStack;              // 0 = the compiled capacity; may only lower it
};
// The node as the costing reads it
struct Node {
    const Edge *mesh; uint32_t nE;                  // compact face ids (CompactNode)
    const float *dirs; uint32_t M;                  // the node's own direction list
    const uint32_t *cdir; uint32_t nD;              // compact direction -> direction, ascending
    const BvhRec *bvh; uint32_t nBvh;               // empty when the node has no plane candidate
    const uint32_t *primOrder, *primNums; uint32_t nPrims;      // ordered position -> local primitive -> primitive
    const float *bmin, *bmax, *tri9; const uint8_t *isTri; uint32_t nTotal;
};
struct Store {
    Q *left, *right, *fv; size_t stride;
    uint8_t *flist; size_t fstride;
    uint32_t *stack; size_t sstride;
    uint32_t capEdges, capFaces, capFaceEdges, capStack;
};
// 16-byte words a lane needs: both halves and the face vertices
constexpr size_t kStoreWords = 4 * (size_t)BSP_MAX_EDGES + 2 * (size_t)BSP_MAX_FACES;

static_assert(BSP_MAX_EDGES <= 128 && BSP_MAX_EDGES % 16 == 0, "the coincident mask has 128 bits, list entries are bytes");
static_assert(BSP_MAX_FACE_EDGES <= 64, "the used mask has 64 bits");
static_assert(BSP_MAX_FACES % 2 == 0 && BSP_MAX_FACES >= 8, "a box and a cut");
static_assert(sizeof(Cand) == 32 && sizeof(BvhRec) == 32 && sizeof(Scalars) == 40, "records shared with the device");

KDOP_HD float fmin_std(float a, float b) { return (b < a) ? b : a; }   // std::min
KDOP_HD float fmax_std(float a, float b) { return (a < b) ? b : a; }   // std::max
KDOP_HD float Inf() { return BitsF(0x7f800000u); }

// One candidate's working state
struct Work {
    Store st;
    uint32_t nLeft, nRight;
    uint64_t coin0, coin1;     // input edges that lie in the plane
    uint32_t p, shift;         // the candidate's compact direction; 2 when it enters the table (faces >= 2 p move up), else 0
    uint32_t id;               // DirectionId: the candidate's place in the node's own list, M when it is new
    bool overflow;
};

KDOP_HD void Push(Work &w, bool right, const Edge &e) {
    uint32_t &n = right ? w.nRight : w.nLeft;
    if (n >= w.st.capEdges) { w.overflow = true; return; }
    StoreEdge(right ? w.st.right : w.st.left, w.st.stride, n, e);
    ++n;
    BSP_NOTE_MAX(0, n);
}

// KDOPCutHelper over two stored points and a saturating count (kdop_cost.h: AddVertex has the argument)
KDOP_HD void AddVertex(Work &w, uint32_t face, const float *p) {
    const size_t S = w.st.stride;
    const Q q0 = w.st.fv[(size_t)(2 * face) * S];
    const uint32_t cnt = q0.w;
    if (cnt == 3) return;
    if (cnt >= 1) {
        const float v[3] = {BitsF(q0.x), BitsF(q0.y), BitsF(q0.z)};
        if (Same(v, p)) return;
    }
    if (cnt == 2) {
        const Q q1 = w.st.fv[(size_t)(2 * face + 1) * S];
        const float v[3] = {BitsF(q1.x), BitsF(q1.y), BitsF(q1.z)};
        if (Same(v, p)) return;
    }
    if (cnt == 0) { w.st.fv[(size_t)(2 * face) * S] = Q{FBits(p[0]), FBits(p[1]), FBits(p[2]), 1u}; return; }
    if (cnt == 1) w.st.fv[(size_t)(2 * face + 1) * S] = Q{FBits(p[0]), FBits(p[1]), FBits(p[2]), 0u};
    w.st.fv[(size_t)(2 * face) * S] = Q{q0.x, q0.y, q0.z, cnt + 1};
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

// The node's edge k with the child's compact face ids
KDOP_HD Edge InputEdge(const Work &w, const Edge *mesh, uint32_t k) {
    Edge e = mesh[k];
    if (e.f1 >= 2 * w.p) e.f1 += w.shift;
    if (e.f2 >= 2 * w.p) e.f2 += w.shift;
    return e;
}

// KDOPCut over the child's nFaces compact faces; the cut's own faces are 2 p (below) and 2 p + 1 (above)
KDOP_HD void Cut(Work &w, const Edge *mesh, uint32_t nE, uint32_t nFaces, float t, const float *direction) {
    w.nLeft = w.nRight = 0; w.coin0 = w.coin1 = 0;
    const uint32_t cutFace = 2 * w.p;
    for (uint32_t i = 0; i < nFaces; ++i) w.st.fv[(size_t)(2 * i) * w.st.stride] = Q{0u, 0u, 0u, 0u};
    for (uint32_t k = 0; k < nE; ++k) {
        const Edge edge = InputEdge(w, mesh, k);
        const float t1 = Dot(direction, edge.v1), t2 = Dot(direction, edge.v2);
        if (t1 > t2) CutAddEdge(w, MakeEdge(edge.v2, edge.v1, edge.f1, edge.f2), k, t, t2, t1);
        else CutAddEdge(w, edge, k, t, t1, t2);
        if (w.overflow) return;
    }
    for (uint32_t k = 0; k < nE; ++k) {
        if (!(((k < 64 ? w.coin0 >> k : w.coin1 >> (k - 64))) & 1u)) continue;
        const Edge edge = InputEdge(w, mesh, k);
        // the first left edge sharing one of its faces decides which half keeps which face (the loop ends at the first match)
        const uint32_t nl = w.nLeft;
        for (uint32_t j = 0; j < nl; ++j) {
            const Q b = w.st.left[(size_t)(2 * j + 1) * w.st.stride];
            const uint32_t lf1 = b.z, lf2 = b.w;
            if (lf1 == edge.f1 || lf2 == edge.f1) {
                Push(w, false, MakeEdge(edge.v1, edge.v2, edge.f1, cutFace));
                Push(w, true, MakeEdge(edge.v1, edge.v2, edge.f2, cutFace + 1));
                break;
            } else if (lf1 == edge.f2 || lf2 == edge.f2) {
                Push(w, false, MakeEdge(edge.v1, edge.v2, edge.f2, cutFace));
                Push(w, true, MakeEdge(edge.v1, edge.v2, edge.f1, cutFace + 1));
                break;
            }
        }
        if (w.overflow) return;
    }
    for (uint32_t i = 0; i < nFaces; ++i) {
        const Q q0 = w.st.fv[(size_t)(2 * i) * w.st.stride];
        if (q0.w != 2u) continue;
        const Q q1 = w.st.fv[(size_t)(2 * i + 1) * w.st.stride];
        const float a[3] = {BitsF(q0.x), BitsF(q0.y), BitsF(q0.z)}, b[3] = {BitsF(q1.x), BitsF(q1.y), BitsF(q1.z)};
        AddEdgeIfNeeded(w, false, MakeEdge(a, b, i, cutFace));
        AddEdgeIfNeeded(w, true, MakeEdge(a, b, i, cutFace + 1));
        if (w.overflow) return;
    }
}

// KDOPSurfaceArea over one half and the child's compact faces (kdop_cost.h: SurfaceArea).  The direction of compact face i is the
// candidate's own for the entered direction, else the node's cdir[] entry
KDOP_HD float SurfaceArea(Work &w, bool right, const Node &nd, float ax, float ay, float az, uint32_t nFaces) {
    Q *base = right ? w.st.right : w.st.left;
    const uint32_t n = right ? w.nRight : w.nLeft;
    const size_t S = w.st.stride, FS = w.st.fstride;
    const uint32_t cap = w.st.capFaceEdges;
    uint8_t *list = w.st.flist;
    float SA = 0;
    for (uint32_t i = 0; i < nFaces; ++i) {
        float fx = 0, fy = 0, fz = 0;
        uint32_t m = 0;
        for (uint32_t k = 0; k < n; ++k) {
            const Q b = base[(size_t)(2 * k + 1) * S];
            if (b.z == i) { if (m >= cap) { w.overflow = true; return 0; } list[m++ * FS] = (uint8_t)k; }
            if (b.w == i) { if (m >= cap) { w.overflow = true; return 0; } list[m++ * FS] = (uint8_t)k; }
        }
        BSP_NOTE_MAX(2, m);
        if (m != 0) {
            uint64_t used = 0;
            uint32_t edgeId = 0;
            // every pass marks a new place, so at most m passes; the bound is the list's capacity
            for (uint32_t pass = 0; pass <= BSP_MAX_FACE_EDGES; ++pass) {
                if ((used >> edgeId) & 1u) break;
                used |= (uint64_t)1 << edgeId;
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
        const uint32_t c = i / 2;
        // The entered direction is the candidate's own axis only when it is new to the node (id == M); one of the node's
        // directions that owns no face of the mesh keeps its own vector.  (The candidate's axis arrives by value: a choice
        // between two pointers would keep the candidate in private memory.)
        float d0 = ax, d1 = ay, d2 = az;
        if (!(w.shift && c == w.p && w.id == nd.M)) {
            const float *nodeDir = nd.dirs + 3 * ((w.shift && c == w.p) ? w.id : nd.cdir[c - ((w.shift && c > w.p) ? 1u : 0u)]);
            d0 = nodeDir[0]; d1 = nodeDir[1]; d2 = nodeDir[2];
        }
        const float s = d0 * fx + d1 * fy + d2 * fz;
        SA += BitsF(FBits(s) & 0x7fffffffu);         // std::abs(float): clears the sign bit
    }
    return SA / 2.0f;
}

// Primitive::getBounds(direction) (bsp_build.h: PrimBounds)
KDOP_HD void PrimBounds(const Node &nd, uint32_t pn, const float *d, float *mnOut, float *mxOut) {
    if (nd.isTri[pn]) {
        const float *v = nd.tri9 + 9 * (size_t)pn;
        float t = Dot(d, v);
        float mn = t, mx = t;
        for (int c = 1; c < 3; ++c) {
            t = Dot(d, v + 3 * c);
            if (t > mx) mx = t;
            else if (t < mn) mn = t;
        }
        *mnOut = mn; *mxOut = mx;
        return;
    }
    float mn = BitsF(0x7f7fffffu), mx = BitsF(0xff7fffffu);      // numeric_limits<float>::max(), lowest()
    const float *bl = nd.bmin + 3 * (size_t)pn, *bh = nd.bmax + 3 * (size_t)pn;
    for (int c = 0; c < 8; ++c) {
        const float q[3] = {(c & 1) ? bh[0] : bl[0], (c & 2) ? bh[1] : bl[1], (c & 4) ? bh[2] : bl[2]};
        const float proj = Dot(d, q);
        if (proj < mn) mn = proj;
        if (proj > mx) mx = proj;
    }
    *mnOut = mn; *mxOut = mx;
}

// NodeBvh::count (getAmountToLeftAndRight): the pop order is the host code's, the second child pushed last.  A well-formed BVH
// pops every node at most once, which bounds the loop.
KDOP_HD void Count(Work &w, const Node &nd, float t, const float *axis, uint32_t *left, uint32_t *right) {
    uint32_t l = 0, r = 0, sp = 1;
    const size_t SS = w.st.sstride;
    if (nd.nBvh == 0 || w.st.capStack == 0) { w.overflow = true; return; }
    w.st.stack[0] = 0;
    for (uint32_t it = 0; it < nd.nBvh && sp > 0; ++it) {
        const uint32_t idx = w.st.stack[(size_t)(--sp) * SS];
        if (idx >= nd.nBvh) { w.overflow = true; return; }
        const BvhRec rec = nd.bvh[idx];
        const float centerProjection = axis[0] * rec.c[0] + axis[1] * rec.c[1] + axis[2] * rec.c[2];
        const uint32_t np = rec.countAxis >> 2;
        if (centerProjection + rec.maxDiff < t) l += np;
        else if (centerProjection - rec.maxDiff > t) r += np;
        else if ((rec.countAxis & 3u) == 3u) {
            const uint32_t first = (uint32_t)rec.offset;
            if (first > nd.nPrims || np > nd.nPrims - first) { w.overflow = true; return; }
            for (uint32_t i = 0; i < np; ++i) {
                const uint32_t local = nd.primOrder[first + i];
                if (local >= nd.nPrims) { w.overflow = true; return; }
                const uint32_t pn = nd.primNums[local];
                if (pn >= nd.nTotal) { w.overflow = true; return; }
                float mn, mx;
                PrimBounds(nd, pn, axis, &mn, &mx);
                if (mn <= t) l += 1;
                if (mx >= t) r += 1;
            }
        } else {
            if (sp + 2 > w.st.capStack) { w.overflow = true; return; }
            w.st.stack[(size_t)sp * SS] = idx + 1;
            w.st.stack[(size_t)(sp + 1) * SS] = (uint32_t)rec.offset;
            sp += 2;
            BSP_NOTE_MAX(3, sp);
        }
    }
    if (sp != 0) { w.overflow = true; return; }
    *left = l; *right = r;
}

// One candidate of costRange.  *cost / *costFixed: what costRange leaves in costs[k] / costsFixed[k] (the latter +inf unless a
// kd-aware plane candidate inside the extent); *nBelow / *nAbove: the candidate's own for an axis candidate or a plane outside the
// extent, else NodeBvh::count's.  Nothing is reported when *overflow is set.
KDOP_HD void CostCandidate(const Node &nd, bool kdAware, const Scalars &sc, const Cand &c, const Store &st, float *cost, float *costFixed,
                           uint32_t *nBelow, uint32_t *nAbove, uint8_t *overflow) {
    Work w;
    w.st = st; w.overflow = false;
    *cost = 0; *costFixed = Inf(); *nBelow = c.nBelow; *nAbove = c.nAbove; *overflow = 1;
    const bool plane = c.k == 33u;
    const float ax = c.axis[0], ay = c.axis[1], az = c.axis[2];
    if (nd.nE > st.capEdges || nd.M > BSP_MAX_DIRS || 2 * nd.nD > st.capFaces) return;
    if (plane) {
        float mn = BitsF(0x7f7fffffu), mx = BitsF(0xff7fffffu);
        for (uint32_t k = 0; k < nd.nE; ++k) {
            const float t1 = Dot(c.axis, nd.mesh[k].v1), t2 = Dot(c.axis, nd.mesh[k].v2);
            mn = fmin_std(mn, fmin_std(t1, t2)); mx = fmax_std(mx, fmax_std(t1, t2));
        }
        if (!(c.t > mn && c.t < mx)) { *cost = Inf(); *overflow = 0; return; }
    }
    // DirectionId: the first of the node's directions within half a degree, else a new one
    uint32_t id = nd.M;
    for (uint32_t i = 0; i < nd.M; ++i)
        if ((double)(nd.dirs[3 * i] * c.axis[0] + nd.dirs[3 * i + 1] * c.axis[1] + nd.dirs[3 * i + 2] * c.axis[2]) > 0.999961923) { id = i; break; }
    uint32_t p = 0;
    while (p < nd.nD && nd.cdir[p] < id) ++p;
    const bool entered = !(p < nd.nD && nd.cdir[p] == id);
    w.p = p; w.shift = entered ? 2u : 0u; w.id = id;
    const uint32_t nFaces = 2 * (nd.nD + (entered ? 1u : 0u));
    BSP_NOTE_MAX(1, nFaces);
    if (nFaces > st.capFaces) return;
    Cut(w, nd.mesh, nd.nE, nFaces, c.t, c.axis);
    float areaBelow = 0, areaAbove = 0;
    if (!w.overflow) areaBelow = SurfaceArea(w, false, nd, ax, ay, az, nFaces);
    if (!w.overflow) areaAbove = SurfaceArea(w, true, nd, ax, ay, az, nFaces);
    uint32_t nb = c.nBelow, na = c.nAbove;
    if (!w.overflow && plane) Count(w, nd, c.t, c.axis, &nb, &na);
    if (w.overflow) return;
    *overflow = 0;
    *nBelow = nb; *nAbove = na;
    const float pBelow = areaBelow * sc.invTotalSA;
    const float pAbove = areaAbove * sc.invTotalSA;
    const float eb = (na == 0 || nb == 0) ? sc.emptyBonus : 0;
    const float BSP_ALPHA = 0.1f;
    if (!kdAware) {
        *cost = (float)sc.traversalCost + (float)sc.isectCost * (1 - eb) * (pBelow * (float)nb + pAbove * (float)na);
    } else if (!plane) {
        *cost = (float)sc.kdTraversalCost + (float)sc.isectCost * (1 - eb) * (pBelow * (float)nb + pAbove * (float)na);
    } else {
        const float costIntersection = (float)sc.isectCost * (1 - eb) * (pBelow * (float)nb + pAbove * (float)na);
        *costFixed = (float)sc.traversalCost + costIntersection;
        *cost = BSP_ALPHA * (float)sc.isectCost * (float)(sc.nPrimitives - 1) + (float)sc.kdTraversalCost + costIntersection;
    }
}

// The capacities a request runs at: the compiled ones, lowered by the scalars' non-zero fields.  False when a field asks for more.
inline bool Capacities(const Scalars &sc, uint32_t cap[4]) {
    const uint32_t compiled[4] = {BSP_MAX_EDGES, BSP_MAX_FACES, BSP_MAX_FACE_EDGES, BSP_MAX_STACK};
    const uint32_t asked[4] = {sc.maxEdges, sc.maxFaces, sc.maxFaceEdges, sc.maxStack};
    for (int k = 0; k < 4; ++k) {
        if (asked[k] > compiled[k]) return false;
        cap[k] = asked[k] ? asked[k] : compiled[k];
    }
    return true;
}

// Host: the node's mesh with compact face ids (out: room for nE edges) and cdir[] (room for M entries); *nD directions own a
// face.  Every face id of the mesh is below 2 M (the caller has checked).  Order-preserving, so the areas add up in the order of
// the vector code.
inline void CompactNode(const Edge *mesh, uint32_t nE, uint32_t M, Edge *out, uint32_t *cdir, uint32_t *nD) {
    uint32_t n = 0;
    for (uint32_t d = 0; d < M; ++d) {
        bool owns = false;
        for (uint32_t k = 0; k < nE && !owns; ++k) owns = mesh[k].f1 / 2 == d || mesh[k].f2 / 2 == d;
        if (owns) cdir[n++] = d;
    }
    for (uint32_t k = 0; k < nE; ++k) {
        out[k] = mesh[k];
        uint32_t *f[2] = {&out[k].f1, &out[k].f2};
        for (uint32_t *x : f) {
            uint32_t r = 0;
            while (cdir[r] != *x / 2) ++r;
            *x = 2 * r + (*x & 1u);
        }
    }
    *nD = n;
}

}  // namespace bspcost
}  // namespace hprt
