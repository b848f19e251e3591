// TEST INFRASTRUCTURE ONLY — a single-threaded restatement of the reference's ambient-occlusion render over the oracle's scene,
// camera, film, sampler and BVH (oracle/orc_integrator.h), in the reference's shape:
//   the array samples   Sampler::Request2DArray / Get2DArray and GlobalSampler::StartPixel / Get1D / Get2D (core/sampler.cpp:66-98, 136-195)
//   AOIntegrator::Li    integrators/ao.cpp:57-103
//   the tile loop       SamplerIntegrator::Render, core/integrator.cpp:230-360
// tests/ao_ref.py compiles and loads it.  Parity of hprt_render_ao is held to THIS file: no reference binary is built here, so the
// restatement itself is unpinned (tests/test_ao_host.py holds it against the oracle's sampler and against geometry).
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
#include "orc_integrator.h"

namespace orc { bool g_use_libm = false; }
using namespace orc;

namespace {

thread_local std::string g_err;

// core/sampling.cpp:89-96
inline V3 UniformSampleHemisphere(const P2 &u) {
    Float z = u.x;
    Float r = std::sqrt(smax((Float)0, (Float)1. - z * z));
    Float phi = 2 * Pi * u.y;
    return V3(r * m_cosf(phi), r * m_sinf(phi), z);
}
inline Float UniformHemispherePdf() { return Inv2Pi; }
// core/sampling.h:165
inline Float CosineHemispherePdf(Float cosTheta) { return cosTheta * InvPi; }

// GlobalSampler over the oracle's HaltonSampler with ONE 2D array of n samples requested (AOIntegrator's constructor, ao.cpp:54):
// arrayStartDim = 5 (core/sampler.h:113), arrayEndDim = 5 + 2 * 1 = 7 (core/sampler.cpp:142-143)
struct ArrayHaltonSampler {
    HaltonSampler h;
    int n;                               // samples2DArraySizes[0]
    std::vector<P2> sampleArray2D;       // [n * samplesPerPixel]
    size_t array2DOffset = 0;
    static const int arrayStartDim = 5;
    int arrayEndDim = 7;
    ArrayHaltonSampler(int spp, int n, int sx0, int sy0, int sx1, int sy1, bool center) : h(spp, sx0, sy0, sx1, sy1, center), n(n) {
        sampleArray2D.assign((size_t)n * (size_t)spp, P2(0, 0));
    }
    void StartPixel(int x, int y) {      // core/sampler.cpp:136-166
        h.StartPixel(x, y);
        array2DOffset = 0;
        arrayEndDim = arrayStartDim + 0 + 2 * 1;
        int dim = arrayStartDim + 0;
        int nSamples = n * (int)h.samplesPerPixel;
        for (int j = 0; j < nSamples; ++j) {
            int64_t idx = h.GetIndexForSample(j);
            sampleArray2D[j].x = h.SampleDimension(idx, dim);
            sampleArray2D[j].y = h.SampleDimension(idx, dim + 1);
        }
    }
    bool StartNextSample() { array2DOffset = 0; return h.StartNextSample(); }      // Sampler::StartNextSample resets the array offsets (core/sampler.cpp:70-75)
    Float Get1D() {                      // core/sampler.cpp:180-185
        if (h.dimension >= arrayStartDim && h.dimension < arrayEndDim) h.dimension = arrayEndDim;
        return h.SampleDimension(h.intervalSampleIndex, h.dimension++);
    }
    P2 Get2D() {                         // core/sampler.cpp:187-195
        if (h.dimension + 1 >= arrayStartDim && h.dimension < arrayEndDim) h.dimension = arrayEndDim;
        P2 p(h.SampleDimension(h.intervalSampleIndex, h.dimension), h.SampleDimension(h.intervalSampleIndex, h.dimension + 1));
        h.dimension += 2;
        return p;
    }
    const P2 *Get2DArray(int count) {    // core/sampler.cpp:93-98
        if (array2DOffset == 1 || count != n) return nullptr;
        ++array2DOffset;
        return &sampleArray2D[(size_t)h.currentPixelSampleIndex * (size_t)n];
    }
};

struct HemisphereRay { Ray ray; Float term; };

// AOIntegrator::Li, integrators/ao.cpp:57-103.  u: Get2DArray's nSamples points.  rays (may be null) receives every generated ray.
Spec AoLi(const Renderer &r, const Ray &camRay, const P2 *u, int nSamples, bool cosSample, Counters &ctr, std::vector<HemisphereRay> *rays,
          int *flipped = nullptr) {
    Spec L(0.f);
    Ray ray(camRay);
    SurfaceInteraction isect;
    if (r.SceneIntersect(ray, &isect, ctr)) {
        // (every material in scope makes a BSDF and there are no media: the "!isect.bsdf" retry of :69-73 never runs)
        V3 n = Faceforward(isect.n, -ray.d);
        V3 s = Normalize(isect.dpdu);
        V3 t = Cross(isect.n, s);
        if (flipped) *flipped = (n.x != isect.n.x || n.y != isect.n.y || n.z != isect.n.z) ? 1 : 0;
        for (int i = 0; i < nSamples; ++i) {
            V3 wi;
            Float pdf;
            if (cosSample) {
                wi = CosineSampleHemisphere(u[i]);
                pdf = CosineHemispherePdf(std::abs(wi.z));
            } else {
                wi = UniformSampleHemisphere(u[i]);
                pdf = UniformHemispherePdf();
            }
            wi = V3(s.x * wi.x + t.x * wi.y + n.x * wi.z, s.y * wi.x + t.y * wi.y + n.y * wi.z, s.z * wi.x + t.z * wi.y + n.z * wi.z);
            Ray shadow = SpawnRay(isect.p, isect.pError, isect.n, wi);
            Float term = Dot(wi, n) / (pdf * nSamples);
            if (rays) rays->push_back(HemisphereRay{shadow, term});
            if (!r.SceneIntersectP(shadow, ctr)) L += Spec(term);
        }
    }
    return L;
}

// One camera sample, core/integrator.cpp:281-324 (minus the film add)
template <class Sampler>
Spec AoRenderSample(const Renderer &r, Sampler &sampler, int px, int py, const P2 *u, int nSamples, bool cosSample, P2 *pFilmOut, Float *rayWeightOut,
                    Counters &ctr, std::vector<HemisphereRay> *rays, int *flipped = nullptr) {
    P2 uf = sampler.Get2D();             // Sampler::GetCameraSample, core/sampler.cpp:46-52
    P2 pFilm((Float)px + uf.x, (Float)py + uf.y);
    Float time = sampler.Get1D(); (void)time;
    P2 pLens = sampler.Get2D();          // dimension 3: the skip test of Get2D is false (3 + 1 < arrayStartDim)
    Ray ray;
    Float rayWeight = r.camera.GenerateRay(pFilm, pLens, &ray);
    ++ctr.cameraRays;
    Spec L(0.f);
    if (rayWeight > 0) L = AoLi(r, ray, u, nSamples, cosSample, ctr, rays, flipped);
    if (L.HasNaNs()) L = Spec(0.f);
    else if (L.y() < -1e-5) L = Spec(0.f);
    else if (std::isinf(L.y())) L = Spec(0.f);
    *pFilmOut = pFilm; *rayWeightOut = rayWeight;
    return L;
}

// A sample taken on its own (sample number s of pixel (x, y), whatever samplesPerPixel is): SetSampleNumber, and the array entries
// Get2DArray would return, formed as StartPixel forms them
struct LoneSample {
    ArrayHaltonSampler sampler;
    std::vector<P2> u;
    LoneSample(const Renderer &r, int nSamples, int x, int y, int64_t s, int sx0, int sy0, int sx1, int sy1)
        : sampler(1, nSamples, sx0, sy0, sx1, sy1, r.scene.prm.samplePixelCenter != 0), u((size_t)nSamples) {
        sampler.h.StartPixel(x, y);
        for (int i = 0; i < nSamples; ++i) {
            int64_t idx = sampler.h.GetIndexForSample(s * nSamples + i);
            u[i].x = sampler.h.SampleDimension(idx, ArrayHaltonSampler::arrayStartDim);
            u[i].y = sampler.h.SampleDimension(idx, ArrayHaltonSampler::arrayStartDim + 1);
        }
        sampler.h.SetSampleNumber(s);
    }
};

void ExportCounters(const Counters &c, uint64_t *o) {      // the layout of oracle_capi.cpp's export_counters
    o[0] = c.nodesFetched; o[1] = c.nodesFetchedP; o[2] = c.nodesEntered; o[3] = c.nodesEnteredP;
    o[4] = c.triTests + c.triTestsPdf; o[5] = c.triTestsP; o[6] = c.triHits + c.triHitsPdf; o[7] = c.triHitsP;
    o[8] = c.sphereTests; o[9] = c.sphereTestsP; o[10] = c.rays; o[11] = c.shadowRays; o[12] = c.cameraRays;
}

}  // namespace

extern "C" {

const char *aoref_last_error() { return g_err.c_str(); }
void *aoref_scene_load(const char *path) {
    Renderer *r = new Renderer();
    std::string err;
    if (!LoadScene(path, &r->scene, &err) || !r->Setup(&err)) { g_err = err; delete r; return nullptr; }
    return r;
}
void aoref_scene_free(void *h) { delete (Renderer *)h; }
// Film and sampler parameters after load: crop as in the scene file (x0 x1 y0 y1 fractions); spp <= 0, center < 0: unchanged
void aoref_set_film(void *h, int xres, int yres, const float *crop4, int spp, int center) {
    Renderer *r = (Renderer *)h;
    if (xres > 0) r->scene.prm.xres = xres;
    if (yres > 0) r->scene.prm.yres = yres;
    if (crop4) for (int i = 0; i < 4; ++i) r->scene.prm.crop[i] = crop4[i];
    if (spp > 0) r->scene.prm.spp = spp;
    if (center >= 0) r->scene.prm.samplePixelCenter = center;
    r->camera.Init(r->scene.prm);
    r->film.Init(r->scene.prm);
}
// out8: croppedPixelBounds x0 y0 x1 y1, sample bounds x0 y0 x1 y1
void aoref_bounds(void *h, int *out8) {
    Renderer *r = (Renderer *)h;
    out8[0] = r->film.cx0; out8[1] = r->film.cy0; out8[2] = r->film.cx1; out8[3] = r->film.cy1;
    r->film.GetSampleBounds(&out8[4], &out8[5], &out8[6], &out8[7]);
}

// SamplerIntegrator::Render (core/integrator.cpp:230-360) over tiles tileBegin, tileBegin + tileStride, ...: film_xyzw = Film::pixels
// (xyz, filterWeightSum) row-major over the cropped pixel bounds, counters13 in the oracle's layout
void aoref_render(void *h, int nSamples, int cosSample, int tileBegin, int tileStride, float *film_xyzw, uint64_t *counters13) {
    Renderer *r = (Renderer *)h;
    const int spp = r->scene.prm.spp;
    int sx0, sy0, sx1, sy1;
    r->film.GetSampleBounds(&sx0, &sy0, &sx1, &sy1);
    for (auto &p : r->film.pixels) p = FilmPixel();
    const int tileSize = 16;
    const int ntx = (sx1 - sx0 + tileSize - 1) / tileSize, nty = (sy1 - sy0 + tileSize - 1) / tileSize;
    Counters ctr;
    ArrayHaltonSampler sampler(spp, nSamples, sx0, sy0, sx1, sy1, r->scene.prm.samplePixelCenter != 0);
    for (int t = tileBegin; t < ntx * nty; t += tileStride) {
        const int tx = t % ntx, ty = t / ntx;
        const int x0 = sx0 + tx * tileSize, x1 = smin(x0 + tileSize, sx1);
        const int y0 = sy0 + ty * tileSize, y1 = smin(y0 + tileSize, sy1);
        FilmTile tile(&r->film, x0, y0, x1, y1);
        for (int y = y0; y < y1; ++y)
            for (int x = x0; x < x1; ++x) {
                sampler.StartPixel(x, y);
                do {
                    // (Li asks for its array after GetCameraSample; the array does not depend on the order)
                    const P2 *u = sampler.Get2DArray(nSamples);
                    P2 pFilm; Float w;
                    Spec L = AoRenderSample(*r, sampler, x, y, u, nSamples, cosSample != 0, &pFilm, &w, ctr, nullptr);
                    tile.AddSample(pFilm, L, w);
                } while (sampler.StartNextSample());
            }
        MergeFilmTile(&r->film, tile);
    }
    for (size_t i = 0; i < r->film.pixels.size(); ++i) {
        const FilmPixel &p = r->film.pixels[i];
        film_xyzw[4 * i] = p.xyz[0]; film_xyzw[4 * i + 1] = p.xyz[1]; film_xyzw[4 * i + 2] = p.xyz[2]; film_xyzw[4 * i + 3] = p.filterWeightSum;
    }
    if (counters13) ExportCounters(ctr, counters13);
}

// L of sample[i] of pixel (px[i], py[i]) after the radiance checks; L3 = 3 * n floats
void aoref_sample(void *h, int nSamples, int cosSample, size_t n, const int32_t *px, const int32_t *py, const int64_t *sample, float *L3) {
    Renderer *r = (Renderer *)h;
    int sx0, sy0, sx1, sy1;
    r->film.GetSampleBounds(&sx0, &sy0, &sx1, &sy1);
    Counters ctr;
    for (size_t i = 0; i < n; ++i) {
        LoneSample ls(*r, nSamples, px[i], py[i], sample[i], sx0, sy0, sx1, sy1);
        P2 pFilm; Float w;
        Spec L = AoRenderSample(*r, ls.sampler, px[i], py[i], ls.u.data(), nSamples, cosSample != 0, &pFilm, &w, ctr, nullptr);
        L3[3 * i] = L.c[0]; L3[3 * i + 1] = L.c[1]; L3[3 * i + 2] = L.c[2];
    }
}

// The hemisphere rays of one camera sample: origin, direction (3 floats each) and term per ray; returns their number (0: the camera
// ray escaped, else nSamples).  index / u (may be null): the Halton index and the two dimensions of each array sample; flipped (may be
// null): 1 where Faceforward(isect.n, -ray.d) differs from isect.n, else 0.
int aoref_rays(void *h, int nSamples, int cosSample, int px, int py, int64_t sample, float *o3, float *d3, float *term, uint64_t *index, float *u2,
               int *flipped) {
    Renderer *r = (Renderer *)h;
    int sx0, sy0, sx1, sy1;
    r->film.GetSampleBounds(&sx0, &sy0, &sx1, &sy1);
    Counters ctr;
    LoneSample ls(*r, nSamples, px, py, sample, sx0, sy0, sx1, sy1);
    for (int i = 0; i < nSamples; ++i) {
        if (index) index[i] = (uint64_t)ls.sampler.h.GetIndexForSample(sample * nSamples + i);
        if (u2) { u2[2 * i] = ls.u[i].x; u2[2 * i + 1] = ls.u[i].y; }
    }
    std::vector<HemisphereRay> rays;
    P2 pFilm; Float w;
    if (flipped) *flipped = 0;
    AoRenderSample(*r, ls.sampler, px, py, ls.u.data(), nSamples, cosSample != 0, &pFilm, &w, ctr, &rays, flipped);
    for (size_t i = 0; i < rays.size(); ++i) {
        o3[3 * i] = rays[i].ray.o.x; o3[3 * i + 1] = rays[i].ray.o.y; o3[3 * i + 2] = rays[i].ray.o.z;
        d3[3 * i] = rays[i].ray.d.x; d3[3 * i + 1] = rays[i].ray.d.y; d3[3 * i + 2] = rays[i].ray.d.z;
        term[i] = rays[i].term;
    }
    return (int)rays.size();
}

// The array samples as the tile loop's sampler holds them after StartPixel(px, py) with the film's samplesPerPixel: u2 = 2 * nSamples * spp
// floats (entry j = s * nSamples + i), and the camera sample's five dimensions of every pixel sample as Get2D / Get1D / Get2D return them
// (cam5 = 5 * spp floats)
void aoref_pixel_samples(void *h, int nSamples, int px, int py, float *u2, float *cam5) {
    Renderer *r = (Renderer *)h;
    int sx0, sy0, sx1, sy1;
    r->film.GetSampleBounds(&sx0, &sy0, &sx1, &sy1);
    const int spp = r->scene.prm.spp;
    ArrayHaltonSampler sampler(spp, nSamples, sx0, sy0, sx1, sy1, r->scene.prm.samplePixelCenter != 0);
    sampler.StartPixel(px, py);
    for (size_t j = 0; j < sampler.sampleArray2D.size(); ++j) { u2[2 * j] = sampler.sampleArray2D[j].x; u2[2 * j + 1] = sampler.sampleArray2D[j].y; }
    int s = 0;
    do {
        P2 a = sampler.Get2D(); Float t = sampler.Get1D(); P2 b = sampler.Get2D();
        cam5[5 * s] = a.x; cam5[5 * s + 1] = a.y; cam5[5 * s + 2] = t; cam5[5 * s + 3] = b.x; cam5[5 * s + 4] = b.y;
        ++s;
    } while (sampler.StartNextSample());
}

}  // extern "C"
