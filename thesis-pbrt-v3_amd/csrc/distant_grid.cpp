// hprt — host build of the light-aligned shadow grid of a distant light (distant_grid.h; the argument for its margins: DESIGN.md §14).
#include "distant_grid.h"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace hprt {

uint32_t DistantGridResFromEnv() {
    const char *e = getenv("HPRT_SHADOW_GRID_RES");
    const long v = e ? atol(e) : (long)DG_DEFAULT_RES;
    return (uint32_t)std::min(2048l, std::max(1l, v));
}

namespace {
inline uint32_t f2u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
inline double dot3(const double a[3], const float b[3]) { return a[0] * (double)b[0] + a[1] * (double)b[1] + a[2] * (double)b[2]; }
}  // namespace

void BuildDistantGrid(const float *tris, const uint8_t *single, uint32_t nPrims, const float w[3], const float bmin[3],
                      const float bmax[3], uint32_t R, size_t maxEntries, double maxCandidates, DistantGrid *out) {
    const auto t0 = std::chrono::steady_clock::now();
    DistantGrid &dg = *out;
    dg = DistantGrid();
    ShadowGrid &g = dg.lists;
    DgFrame &F = dg.frame;
    const double wl = std::sqrt((double)w[0] * w[0] + (double)w[1] * w[1] + (double)w[2] * w[2]);
    if (!(wl > 0.5 && wl < 2.0)) return;      // (a direction that is not finite, or not normalised: the scene keeps the walk)
    for (int a = 0; a < 3; ++a) { g.light[a] = w[a]; F.W[a] = w[a]; }
    // U = e x w / |e x w| with e the axis of w's smallest |component| (ties to the lower axis), V = w x U / |w x U|: in double, stored
    // as floats; the build reads the floats back, so host and device project onto the same vectors
    int ax = 0;
    for (int a = 1; a < 3; ++a) if (std::fabs(w[a]) < std::fabs(w[ax])) ax = a;
    double e[3] = {0, 0, 0}, U[3], V[3];
    e[ax] = 1.0;
    const double W[3] = {w[0], w[1], w[2]};
    U[0] = e[1] * W[2] - e[2] * W[1]; U[1] = e[2] * W[0] - e[0] * W[2]; U[2] = e[0] * W[1] - e[1] * W[0];
    const double ul = std::sqrt(U[0] * U[0] + U[1] * U[1] + U[2] * U[2]);
    for (int a = 0; a < 3; ++a) U[a] /= ul;
    V[0] = W[1] * U[2] - W[2] * U[1]; V[1] = W[2] * U[0] - W[0] * U[2]; V[2] = W[0] * U[1] - W[1] * U[0];
    const double vl = std::sqrt(V[0] * V[0] + V[1] * V[1] + V[2] * V[2]);
    for (int a = 0; a < 3; ++a) { V[a] /= vl; F.U[a] = (float)U[a]; F.V[a] = (float)V[a]; }
    // extent: no coordinate of an origin in the bound, of T = p + w * 2 worldRadius or of d = T - o is larger
    double coord = 0, diag2 = 0;
    for (int a = 0; a < 3; ++a) {
        coord = std::max(coord, std::max(std::fabs((double)bmin[a]), std::fabs((double)bmax[a])));
        diag2 += ((double)bmax[a] - bmin[a]) * ((double)bmax[a] - bmin[a]);
    }
    const double extent = coord + std::sqrt(diag2);
    if (!std::isfinite(extent) || !(extent > 0)) { dg = DistantGrid(); return; }
    const double eps = SG_EPS_FACTOR * std::ldexp(1.0, -23) * extent;
    const double margin = DG_MARGIN_EPS * eps, hMargin = DG_HEIGHT_EPS * eps;
    g.eps = eps; dg.margin = margin; dg.heightMargin = hMargin;
    // the bound's projection: the rectangle of the cells, and the top height the keys are measured down from
    double lo[2] = {1e300, 1e300}, hi[2] = {-1e300, -1e300}, top = -1e300;
    for (int c = 0; c < 8; ++c) {
        const double p[3] = {(c & 1) ? bmax[0] : bmin[0], (c & 2) ? bmax[1] : bmin[1], (c & 4) ? bmax[2] : bmin[2]};
        const double u = dot3(p, F.U), v = dot3(p, F.V);
        lo[0] = std::min(lo[0], u); hi[0] = std::max(hi[0], u); lo[1] = std::min(lo[1], v); hi[1] = std::max(hi[1], v);
        top = std::max(top, dot3(p, F.W));
    }
    F.u0 = (float)(lo[0] - margin); F.v0 = (float)(lo[1] - margin);
    F.hTop = std::nextafter((float)(top + hMargin), HUGE_VALF);      // (never below top + hMargin: a key is never negative before it is cut)
    const double sideU = std::max(hi[0] - lo[0] + 2 * margin, 64 * eps), sideV = std::max(hi[1] - lo[1] + 2 * margin, 64 * eps);
    std::vector<SgEntry> nearList;
    struct Cover { uint32_t prim, key; double u0, u1, v0, v1; };
    std::vector<Cover> covers;
    covers.reserve(nPrims);
    for (uint32_t i = 0; i < nPrims; ++i) {
        const float *t = tris + 12 * (size_t)i;
        const uint32_t word = i | ((single && single[i]) ? SG_SINGLE : 0u);
        double r[4] = {1e300, -1e300, 1e300, -1e300}, h = -1e300;
        bool finite = true;
        for (int k = 0; k < 3; ++k) {
            const double p[3] = {t[4 * k], t[4 * k + 1], t[4 * k + 2]};
            finite = finite && std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]);
            const double u = dot3(p, F.U), v = dot3(p, F.V);
            r[0] = std::min(r[0], u); r[1] = std::max(r[1], u); r[2] = std::min(r[2], v); r[3] = std::max(r[3], v);
            h = std::max(h, dot3(p, F.W));
        }
        if (!finite) { nearList.push_back({word, SG_RECT_ALL}); continue; }
        // the key: how far the triangle's top, raised by the margin, lies below hTop, as a float rounded down (two ulps below the
        // nearest float; an entry keeps its upper 16 bits: down again)
        const float kf = (float)std::max(0.0, (double)F.hTop - h - hMargin);
        uint32_t kb = f2u(kf); kb = kb >= 2u ? kb - 2u : 0u;
        covers.push_back({word, kb, r[0] - margin, r[1] + margin, r[2] - margin, r[3] + margin});
    }
    g.nNear = (uint32_t)nearList.size();
    // the cost model (shadow_grid.h): a near list that long alone settles it, before any list is laid out
    if (maxCandidates > 0 && (double)nearList.size() > maxCandidates) { dg = DistantGrid(); return; }
    for (;; R = std::max(1u, R / 2)) {
        // a side holds 16 R fine columns: the cell is the fine column's upper bits, its lower four bits say where in the cell.  The
        // scales are floats, as the device multiplies by them
        F.scaleU = (float)(16.0 * R / sideU); F.scaleV = (float)(16.0 * R / sideV);
        const double u0 = F.u0, v0 = F.v0, su = F.scaleU, sv = F.scaleV;
        auto fine = [&](double x, double x0, double s) { const double c = std::floor((x - x0) * s); return (uint32_t)std::min(16.0 * R - 1.0, std::max(0.0, c)); };
        const size_t nCells = (size_t)R * R;
        std::vector<uint32_t> count(nCells + 1, 0u);
        size_t total = 0;
        bool over = false;
        for (const Cover &c : covers) {
            const uint32_t iu0 = fine(c.u0, u0, su) >> 4, iu1 = fine(c.u1, u0, su) >> 4, iv0 = fine(c.v0, v0, sv) >> 4, iv1 = fine(c.v1, v0, sv) >> 4;
            total += (size_t)(iu1 - iu0 + 1) * (iv1 - iv0 + 1);
            if (total > maxEntries) { over = true; break; }
            for (uint32_t iv = iv0; iv <= iv1; ++iv) for (uint32_t iu = iu0; iu <= iu1; ++iu) ++count[(size_t)iv * R + iu];
        }
        if (over && R > 1) continue;
        if (over) { dg = DistantGrid(); return; }      // (not even one cell fits: the scene keeps the walk)
        if (maxCandidates > 0 && (double)nearList.size() + (double)total / (double)nCells > maxCandidates) { dg = DistantGrid(); return; }      // (counted, not yet filled or sorted)
        g.R = R;
        g.cellStart.assign(nCells + 1, 0u);
        uint32_t at = g.nNear;
        for (size_t c = 0; c < nCells; ++c) { g.cellStart[c] = at; at += count[c]; g.longest = std::max(g.longest, count[c]); }
        g.cellStart[nCells] = at;
        g.entries.resize(at);
        std::copy(nearList.begin(), nearList.end(), g.entries.begin());
        std::vector<uint32_t> fill(g.cellStart.begin(), g.cellStart.end() - 1);
        for (const Cover &c : covers) {
            const uint32_t fu0 = fine(c.u0, u0, su), fu1 = fine(c.u1, u0, su), fv0 = fine(c.v0, v0, sv), fv1 = fine(c.v1, v0, sv);
            for (uint32_t iv = fv0 >> 4; iv <= fv1 >> 4; ++iv)
                for (uint32_t iu = fu0 >> 4; iu <= fu1 >> 4; ++iu) {
                    // the part of the cell the widened rectangle reaches, in sixteenths of the cell
                    const uint32_t su0 = iu == fu0 >> 4 ? fu0 & 15u : 0u, su1 = iu == fu1 >> 4 ? fu1 & 15u : 15u;
                    const uint32_t sv0 = iv == fv0 >> 4 ? fv0 & 15u : 0u, sv1 = iv == fv1 >> 4 ? fv1 & 15u : 15u;
                    g.entries[fill[(size_t)iv * R + iu]++] = {c.prim, (c.key & SG_KEY_MASK) | su0 | (su1 << 4) | (sv0 << 8) | (sv1 << 12)};
                }
        }
        for (size_t c = 0; c < nCells; ++c)
            std::sort(g.entries.begin() + g.cellStart[c], g.entries.begin() + g.cellStart[c + 1],
                      [](const SgEntry &a, const SgEntry &b) { return (a.key & SG_KEY_MASK) != (b.key & SG_KEY_MASK) ? (a.key & SG_KEY_MASK) < (b.key & SG_KEY_MASK) : (a.prim & SG_PRIM_MASK) < (b.prim & SG_PRIM_MASK); });
        break;
    }
    g.eligible = true;
    g.buildSeconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace hprt
