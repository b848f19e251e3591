// hprt — the light-aligned candidate grid of distant-light shadow rays: seen along the light's direction w every
// shadow ray is (almost) a point, so one face of R x R cells, laid over the scene bound's projection onto a frame (U, V) ⟂ w,
// replaces the six faces of the point light's grid (shadow_grid.h).  A cell lists the triangles a shadow ray whose origin projects
// into it could be reported to hit, highest along w first.  k_distant_grid (device/distant_grid.hip) runs the walk's own triangle
// and leaf-box tests over that list.  Entries, keys, rectangles, the near list and the device image are those of shadow_grid.h.
// Host only, no HIP runtime call; hprt_scene_create uploads the result.
#pragma once
#include "shadow_grid.h"

namespace hprt {

// What host and device compute a ray's cell and key limit from — floats, the host reads them back as doubles:
//   fu = clamp(floor((dot(o, U) - u0) * scaleU), 0, 16 R - 1), likewise fv: the cell is the upper bits, the sixteenth the lower four
//   lim = hTop - dot(o, W): an entry is tested while key <= lim (tMax <= 1)
// dot(a, b) = a.x b.x + a.y b.y + a.z b.z, summed left to right, every operation rounded once.
struct DgFrame { float U[3], V[3], W[3], u0, v0, scaleU, scaleV, hTop; };

// The margins, in units of ε = SG_EPS_FACTOR * 2^-23 * extent (32 x the C = 4 of tri_test); extent = the largest
// |coordinate| of the scene bound + its diagonal (= 2 worldRadius), which bounds every coordinate of o, T and d.  DESIGN.md §14
// derives C = 24 for the footprint (tri_test 4, the ray's lateral drift 11.3, the device's projection 6.1) and C = 12 for the height.
constexpr double DG_MARGIN_EPS = 6.0, DG_HEIGHT_EPS = 3.0;
constexpr uint32_t DG_DEFAULT_RES = 1024u;

struct DistantGrid {
    ShadowGrid lists;      // eligible, R, cellStart (R^2 + 1: cell = iv * R + iu), entries, nNear, longest, eps, buildSeconds; light = w
    DgFrame frame{};
    double margin = 0, heightMargin = 0;
};

// A scene has no grid, the point light's (lists alone) or the distant light's
enum class GridKind { None, Point, Distant };

// tris, single, bmin / bmax, R, maxEntries, maxCandidates: as BuildShadowGrid takes them.  w: the direction towards the light
// (LightDesc::pos of a distant light, normalised in float).  A triangle with a vertex that is not finite goes to the near list;
// every other one — edge-on to the light or degenerate too: a segment's or a point's widened rectangle — to the cells.
void BuildDistantGrid(const float *tris, const uint8_t *single, uint32_t nPrims, const float w[3], const float bmin[3],
                      const float bmax[3], uint32_t R, size_t maxEntries, double maxCandidates, DistantGrid *out);

// HPRT_SHADOW_GRID_RES, or DG_DEFAULT_RES
uint32_t DistantGridResFromEnv();

}  // namespace hprt
