// hprt — what the builders of the fork's BSP trees over BSPNode / BSPKdNode share (bsppaper_builder.cpp, bspnode_builder.cpp): the
// vector helpers with pbrt's roundings, PositiveX, Primitive::getBounds, the sweep's edge and build-node types and the cut of a
// k-DOP that carries its own directions (KDOPMeshWithDirections, kDOPMesh.h:238-266).  Every float operation is one IEEE rounding
// in the reference's order (built with -ffp-contract=off).  Host only, header-only.
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>
#include "kdop_mesh.h"

namespace hprt {
namespace bspbuild {

using namespace kdop;

struct V { float x, y, z; };
inline float Length(const V &v) { return std::sqrt(v.x * v.x + v.y * v.y + v.z * v.z); }
inline V Normalize(const V &v) { const float inv = (float)1 / Length(v); return V{v.x * inv, v.y * inv, v.z * inv}; }   // v / v.Length()
inline V Cross(const V &a, const V &b) {      // core/geometry.h: in double, rounded to float
    const double ax = a.x, ay = a.y, az = a.z, bx = b.x, by = b.y, bz = b.z;
    return V{(float)((ay * bz) - (az * by)), (float)((az * bx) - (ax * bz)), (float)((ax * by) - (ay * bx))};
}
inline V Sub(const float *p, const float *q) { return V{p[0] - q[0], p[1] - q[1], p[2] - q[2]}; }
inline float DotP(const V &d, const float *p) { return d.x * p[0] + d.y * p[1] + d.z * p[2]; }
// PositiveX (core/geometry.h:1849-1862)
inline V PositiveX(const V &v) {
    if (v.x > 0) return Normalize(v);
    if (v.x == 0) {
        if (v.y == 0) return Normalize(V{0, 0, 1});
        const float s = (v.y > 0) ? 1 : -1;
        return Normalize(V{0, v.y / s, v.z / s});
    }
    return Normalize(V{-v.x, -v.y, -v.z});
}

struct Range { float min, max; };             // Boundsf: {max, lowest} when empty

// Primitive::getBounds(direction): Triangle::getBounds (shapes/triangle.cpp:661-676) or the world bound's 8 corners (core/shape.h:103-113)
inline Range PrimBounds(const float *bmin, const float *bmax, const float *tri9, const uint8_t *isTri, uint32_t pn, const float *d) {
    if (isTri[pn]) {
        const float *v = tri9 + 9 * (size_t)pn;
        float t = Dot(d, P3{v[0], v[1], v[2]});
        float mn = t, mx = t;
        for (int c = 1; c < 3; ++c) {
            t = Dot(d, P3{v[3 * c], v[3 * c + 1], v[3 * c + 2]});
            if (t > mx) mx = t;
            else if (t < mn) mn = t;
        }
        return Range{mn, mx};
    }
    Range b{std::numeric_limits<float>::max(), std::numeric_limits<float>::lowest()};
    const float *bl = bmin + 3 * (size_t)pn, *bh = bmax + 3 * (size_t)pn;
    for (int c = 0; c < 8; ++c) {
        const float proj = Dot(d, P3{(c & 1) ? bh[0] : bl[0], (c & 2) ? bh[1] : bl[1], (c & 4) ? bh[2] : bl[2]});
        if (proj < b.min) b.min = proj;
        if (proj > b.max) b.max = proj;
    }
    return b;
}

enum class EdgeType : int { Start, End };
struct BoundEdge { float t; uint32_t primNum; EdgeType type; };     // accelerators/genericBSP.h:47-58
struct BuildNode {                                                  // BSPBuildNode: the k-DOP carries its own directions
    uint32_t depth, nPrimitives, badRefines;
    Mesh mesh; std::vector<float> dirs; float meshArea;
    size_t primNums; uint32_t parentNum;                            // primNums: offset into `prims`
};

inline int Log2Int64(uint64_t v) { return v ? 63 - __builtin_clzll(v) : -1; }

// KDOPMeshWithDirections::cut's direction: the first of the mesh's directions with Dot > cos(0.5 degrees), else a new one
inline uint32_t DirectionId(const std::vector<float> &dirs, const float *d) {
    const uint32_t M = (uint32_t)(dirs.size() / 3);
    for (uint32_t i = 0; i < M; ++i)
        if ((double)(dirs[3 * i] * d[0] + dirs[3 * i + 1] * d[1] + dirs[3 * i + 2] * d[2]) > 0.999961923) return i;
    return M;
}
// cut + the two SurfaceArea calls of a candidate: the halves (reoriented by SurfaceArea) in s.left / s.right, their directions in *childDirs
inline void CutMeasure(const BuildNode &cur, float t, const float *d, Scratch &s, std::vector<float> *childDirs, float *areaBelow, float *areaAbove) {
    const uint32_t M = (uint32_t)(cur.dirs.size() / 3);
    const uint32_t id = DirectionId(cur.dirs, d);
    Cut(cur.mesh, M, t, d, id, s);
    *childDirs = cur.dirs;
    if (id == M) childDirs->insert(childDirs->end(), d, d + 3);
    const uint32_t Mc = (uint32_t)(childDirs->size() / 3);
    *areaBelow = SurfaceArea(s.left, childDirs->data(), Mc, s);
    *areaAbove = SurfaceArea(s.right, childDirs->data(), Mc, s);
}

}  // namespace bspbuild
}  // namespace hprt
