// hprt — host build of the light-centred shadow grid (shadow_grid.h; the argument for its margins: DESIGN.md §11).
#include "shadow_grid.h"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace hprt {

int ShadowGridModeFromEnv() { const char *e = getenv("HPRT_SHADOW_GRID"); return !e ? -1 : atoi(e) == 0 ? 0 : 1; }
uint32_t ShadowGridResFromEnv() {
    const char *e = getenv("HPRT_SHADOW_GRID_RES");
    const long v = e ? atol(e) : (long)SG_DEFAULT_RES;
    return (uint32_t)std::min(2048l, std::max(1l, v));
}

namespace {

struct D3 { double x, y, z; };
inline D3 operator-(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline D3 operator+(D3 a, D3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline D3 operator*(D3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
inline double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline D3 cross(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline double comp(D3 a, int k) { return k == 0 ? a.x : k == 1 ? a.y : a.z; }

// squared distance from the origin to the segment ab
double seg_dist2(D3 a, D3 b) {
    const D3 ab = b - a;
    const double l2 = dot(ab, ab);
    double t = l2 > 0 ? -dot(a, ab) / l2 : 0.0;
    t = std::min(1.0, std::max(0.0, t));
    const D3 p = a + ab * t;
    return dot(p, p);
}
// squared distance from the origin to the triangle abc: the plane's foot point if it lies inside, else the nearest edge
double tri_dist2(D3 a, D3 b, D3 c) {
    double best = std::min(seg_dist2(a, b), std::min(seg_dist2(b, c), seg_dist2(c, a)));
    const D3 n = cross(b - a, c - a);
    const double n2 = dot(n, n);
    if (n2 > 0) {
        const double s = dot(a, n) / n2;
        const D3 q = n * s;      // the foot of the origin on the plane
        const double e0 = dot(cross(b - a, q - a), n), e1 = dot(cross(c - b, q - b), n), e2 = dot(cross(a - c, q - c), n);
        if (e0 >= 0 && e1 >= 0 && e2 >= 0) best = std::min(best, dot(q, q));
    }
    return best;
}

// The bounding rectangle, in the face's (u, v), of the part of the polygon in front of the plane m = lam of face f
// (m: the face's major component, positive on the face's side); false if nothing is
bool face_rect(const D3 *poly, int n, int f, double lam, double r[4]) {
    const int ax = f >> 1; const double sg = (f & 1) ? -1.0 : 1.0;
    D3 out[8]; int no = 0;
    for (int i = 0; i < n; ++i) {
        const D3 p = poly[i], q = poly[(i + 1) % n];
        const double mp = sg * comp(p, ax) - lam, mq = sg * comp(q, ax) - lam;
        if (mp >= 0) out[no++] = p;
        if ((mp >= 0) != (mq >= 0)) { const double t = mp / (mp - mq); out[no++] = p + (q - p) * t; }
    }
    if (no == 0) return false;
    r[0] = r[2] = 1e300; r[1] = r[3] = -1e300;
    for (int i = 0; i < no; ++i) {
        const double m = std::max(sg * comp(out[i], ax), lam);      // (a clipped point sits on the plane up to rounding)
        const double u = comp(out[i], (ax + 1) % 3) / m, v = comp(out[i], (ax + 2) % 3) / m;
        r[0] = std::min(r[0], u); r[1] = std::max(r[1], u); r[2] = std::min(r[2], v); r[3] = std::max(r[3], v);
    }
    return true;
}

inline uint32_t f2u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

}  // namespace

void BuildShadowGrid(const float *tris, const uint8_t *single, uint32_t nPrims, const float light[3], const float bmin[3],
                     const float bmax[3], uint32_t R, size_t maxEntries, double maxCandidates, ShadowGrid *out) {
    const auto t0 = std::chrono::steady_clock::now();
    ShadowGrid &g = *out;
    g = ShadowGrid();
    for (int a = 0; a < 3; ++a) g.light[a] = light[a];
    // extent of the scene bound united with the light: no component of p - o, o in the bound, is larger
    double extent = 0;
    for (int a = 0; a < 3; ++a) extent = std::max(extent, (double)std::max(bmax[a], light[a]) - (double)std::min(bmin[a], light[a]));
    const double eps = SG_EPS_FACTOR * std::ldexp(1.0, -23) * extent;
    g.eps = eps;
    const D3 L = {light[0], light[1], light[2]};
    std::vector<SgEntry> nearList;
    struct Cover { uint32_t prim, key; double u0, u1, v0, v1; uint16_t face; };
    std::vector<Cover> covers;
    covers.reserve((size_t)nPrims * 2);
    for (uint32_t i = 0; i < nPrims; ++i) {
        const float *t = tris + 12 * (size_t)i;
        const D3 v[3] = {D3{t[0], t[1], t[2]} - L, D3{t[4], t[5], t[6]} - L, D3{t[8], t[9], t[10]} - L};
        const uint32_t word = i | ((single && single[i]) ? SG_SINGLE : 0u);
        const D3 n = cross(v[1] - v[0], v[2] - v[0]);
        const double d2 = tri_dist2(v[0], v[1], v[2]);
        const double D = std::sqrt(d2) - eps;      // no point a reported hit can lie at is nearer to the light
        const bool finite = std::isfinite(d2) && std::isfinite(dot(n, n));
        const double margin = D > 0 ? 4.0 * eps / D + std::ldexp(1.0, -20) : 1e300;
        if (!finite || dot(n, n) == 0 || !(D > 0) || margin > 0.5) { nearList.push_back({word, SG_RECT_ALL}); continue; }
        // the key: D^2 as a float rounded down (two ulps below the nearest float; an entry keeps its upper 16 bits: down again)
        float kf = (float)(D * D);
        uint32_t kb = f2u(kf); kb = kb >= 2u ? kb - 2u : 0u;
        const double lam = D / 4;      // a point p inside a face's widened pyramid (|u|, |v| <= 1.5) has m >= |p| / 2.35 > D / 4
        for (int f = 0; f < 6; ++f) {
            double r[4];
            if (!face_rect(v, 3, f, lam, r)) continue;
            r[0] -= margin; r[1] += margin; r[2] -= margin; r[3] += margin;
            if (r[1] < -1 || r[0] > 1 || r[3] < -1 || r[2] > 1) continue;
            covers.push_back({word, kb, r[0], r[1], r[2], r[3], (uint16_t)f});
        }
    }
    g.nNear = (uint32_t)nearList.size();
    // the cost model (shadow_grid.h): a near list that long alone settles it, before any list is laid out
    if (maxCandidates > 0 && (double)nearList.size() > maxCandidates) { g = ShadowGrid(); return; }
    for (;; R = std::max(1u, R / 2)) {
        // a face side holds 16 R fine columns: the cell is the fine column's upper bits, its lower four bits say where in the cell
        const double fineScale = 8.0 * R;
        auto fine = [&](double u) { const double c = std::floor((u + 1.0) * fineScale); return (uint32_t)std::min(16.0 * R - 1.0, std::max(0.0, c)); };
        const size_t nCells = (size_t)6 * R * R;
        std::vector<uint32_t> count(nCells + 1, 0u);
        size_t total = 0;
        bool over = false;
        for (const Cover &c : covers) {
            const uint32_t iu0 = fine(c.u0) >> 4, iu1 = fine(c.u1) >> 4, iv0 = fine(c.v0) >> 4, iv1 = fine(c.v1) >> 4;
            total += (size_t)(iu1 - iu0 + 1) * (iv1 - iv0 + 1);
            if (total > maxEntries) { over = true; break; }
            for (uint32_t iv = iv0; iv <= iv1; ++iv) for (uint32_t iu = iu0; iu <= iu1; ++iu) ++count[((size_t)c.face * R + iv) * R + iu];
        }
        if (over && R > 1) continue;
        if (over) { g = ShadowGrid(); return; }      // (not even one cell per face fits: the scene keeps the walk)
        if (maxCandidates > 0 && (double)nearList.size() + (double)total / (double)nCells > maxCandidates) { g = ShadowGrid(); return; }      // (counted, not yet filled or sorted)
        g.R = R;
        g.cellStart.assign(nCells + 1, 0u);
        uint32_t at = g.nNear;
        for (size_t c = 0; c < nCells; ++c) { g.cellStart[c] = at; at += count[c]; g.longest = std::max(g.longest, count[c]); }
        g.cellStart[nCells] = at;
        g.entries.resize(at);
        std::copy(nearList.begin(), nearList.end(), g.entries.begin());
        std::vector<uint32_t> fill(g.cellStart.begin(), g.cellStart.end() - 1);
        for (const Cover &c : covers) {
            const uint32_t fu0 = fine(c.u0), fu1 = fine(c.u1), fv0 = fine(c.v0), fv1 = fine(c.v1);
            for (uint32_t iv = fv0 >> 4; iv <= fv1 >> 4; ++iv)
                for (uint32_t iu = fu0 >> 4; iu <= fu1 >> 4; ++iu) {
                    // the part of the cell the widened rectangle reaches, in sixteenths of the cell
                    const uint32_t su0 = iu == fu0 >> 4 ? fu0 & 15u : 0u, su1 = iu == fu1 >> 4 ? fu1 & 15u : 15u;
                    const uint32_t sv0 = iv == fv0 >> 4 ? fv0 & 15u : 0u, sv1 = iv == fv1 >> 4 ? fv1 & 15u : 15u;
                    g.entries[fill[((size_t)c.face * R + iv) * R + iu]++] = {c.prim, (c.key & SG_KEY_MASK) | su0 | (su1 << 4) | (sv0 << 8) | (sv1 << 12)};
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

size_t ShadowGridImageBytes(const ShadowGrid &g) {
    const size_t nCells = g.cellStart.empty() ? 0 : g.cellStart.size() - 1;
    size_t nRecords = g.nNear;
    for (size_t c = 0; c < nCells; ++c) {
        const uint32_t n = g.cellStart[c + 1] - g.cellStart[c];
        if (n > SG_BLOCK_SLOTS) nRecords += n - SG_BLOCK_SLOTS;
    }
    return (nCells * SG_BLOCK_WORDS + (nRecords + SG_PAD_RECORDS) * SG_RECORD_WORDS) * sizeof(uint32_t);
}

void PackShadowGrid(const ShadowGrid &g, const float *tris, ShadowGridImage *out) {
    const auto t0 = std::chrono::steady_clock::now();
    ShadowGridImage &im = *out;
    im = ShadowGridImage();
    im.R = g.R; im.nNear = g.nNear;
    const size_t nCells = g.cellStart.empty() ? 0 : g.cellStart.size() - 1;      // faces * R^2: six faces here, one in distant_grid.h
    im.nRecords =(ShadowGridImageBytes(g) / sizeof(uint32_t) - nCells * SG_BLOCK_WORDS) / SG_RECORD_WORDS - SG_PAD_RECORDS;
    im.blocks.assign(nCells * SG_BLOCK_WORDS, 0u);
    im.records.assign((im.nRecords + SG_PAD_RECORDS) * SG_RECORD_WORDS, 0u);
    // a vertex and the word that rides in its fourth lane
    auto put = [&](uint32_t *w, const SgEntry &e, int vertex, uint32_t fourth) {
        memcpy(w, tris + 12 * (size_t)(e.prim & SG_PRIM_MASK) + 4 * vertex, 12);
        w[3] = fourth;
    };
    // entries[a .. b) as one run of records at record `at`
    auto run = [&](size_t at, uint32_t a, uint32_t b) {
        for (uint32_t k = a; k < b; ++k, ++at) {
            uint32_t *w = im.records.data() + at * SG_RECORD_WORDS;
            const SgEntry &e = g.entries[k];
            put(w, e, 0, e.prim); put(w + 4, e, 1, e.key); put(w + 8, e, 2, k + 1 < b ? g.entries[k + 1].key : 0u);
        }
        return at;
    };
    size_t at = run(0, 0u, g.nNear);
    for (size_t c = 0; c < nCells; ++c) {
        const uint32_t a = g.cellStart[c], n = g.cellStart[c + 1] - a;
        uint32_t *w = im.blocks.data() + c * SG_BLOCK_WORDS;
        const SgEntry *e = g.entries.data() + a;
        w[0] = n; w[1] = (uint32_t)at;
        if (n > 0) {
            w[2] = e[0].prim; w[3] = e[0].key;
            put(w + 4, e[0], 0, n > 1 ? e[1].prim : 0u); put(w + 8, e[0], 1, n > 1 ? e[1].key : 0u); put(w + 12, e[0], 2, n > 2 ? e[2].key : 0u);
        }
        if (n > 1) { put(w + 16, e[1], 0, 0u); put(w + 20, e[1], 1, 0u); put(w + 24, e[1], 2, 0u); }
        if (n > SG_BLOCK_SLOTS) at = run(at, a + SG_BLOCK_SLOTS, a + n);
    }
    im.packSeconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace hprt
