// TEST INFRASTRUCTURE ONLY — a single-threaded restatement of the reference's direct-lighting render over the oracle's scene, camera,
// film, sampler, BVH, BSDF and EstimateDirect (oracle/orc_integrator.h), in the reference's shape:
//   the sample arrays          Sampler::Request2DArray / Get2DArray and GlobalSampler::StartPixel / Get1D / Get2D (core/sampler.cpp:80-98, 136-195)
//   Preprocess, Li             DirectLightingIntegrator, integrators/directlighting.cpp:45-100
//   UniformSampleAllLights     core/integrator.cpp:55-84; UniformSampleOneLight without a distribution, :86-107
//   SpecularReflect / Transmit core/integrator.cpp:362-450 (without the child's ray differentials: they decide texture filter widths
//                              only, and the scenes where a child could meet an image texture are refused by hprt_render_direct)
//   the tile loop              SamplerIntegrator::Render, core/integrator.cpp:230-360
// over the oracle's pinned EstimateDirect, Sample_Li / Pdf_Li, masked BSDF::Sample_f, SceneIntersect / SceneIntersectP and film.
// One thing is restated against the oracle's pinned shape: DirectLightingIntegrator::Li calls ComputeScatteringFunctions with
// allowMultipleLobes = false (directlighting.cpp:75, core/interaction.h:132), under which smooth glass is a SpecularReflection and a
// SpecularTransmission lobe (materials/glass.cpp:62-90), not the one FresnelSpecular lobe the oracle builds for the path integrator.
// tests/dl_ref.py compiles and loads it.  Parity of hprt_render_direct is held to THIS file: no reference binary is built here, so the
// restatement itself is unpinned (tests/test_dl_host.py holds it against the oracle's sampler and against known answers).
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>
#include "orc_integrator.h"

namespace orc { bool g_use_libm = false; }
using namespace orc;

namespace {

thread_local std::string g_err;

// GlobalSampler over the oracle's HaltonSampler with the requested 2D arrays: arrayStartDim = 5 (core/sampler.h:113),
// arrayEndDim = 5 + 2 * (number of arrays) (core/sampler.cpp:142-143)
struct DlSampler {
    HaltonSampler h;
    std::vector<int> samples2DArraySizes;
    std::vector<std::vector<P2>> sampleArray2D;
    size_t array2DOffset = 0;
    static const int arrayStartDim = 5;
    int arrayEndDim = 5;
    DlSampler(int spp, int sx0, int sy0, int sx1, int sy1, bool center) : h(spp, sx0, sy0, sx1, sy1, center) {}
    void Request2DArray(int n) {         // core/sampler.cpp:80-84 (Halton's RoundCount is the identity)
        samples2DArraySizes.push_back(n);
        sampleArray2D.push_back(std::vector<P2>((size_t)n * (size_t)h.samplesPerPixel));
    }
    void StartPixel(int x, int y) {      // core/sampler.cpp:136-166
        h.StartPixel(x, y);
        array2DOffset = 0;
        arrayEndDim = arrayStartDim + 0 + 2 * (int)sampleArray2D.size();
        int dim = arrayStartDim + 0;
        for (size_t i = 0; i < samples2DArraySizes.size(); ++i) {
            int nSamples = samples2DArraySizes[i] * (int)h.samplesPerPixel;
            for (int j = 0; j < nSamples; ++j) {
                int64_t idx = h.GetIndexForSample(j);
                sampleArray2D[i][j].x = h.SampleDimension(idx, dim);
                sampleArray2D[i][j].y = h.SampleDimension(idx, dim + 1);
            }
            dim += 2;
        }
    }
    bool StartNextSample() { array2DOffset = 0; return h.StartNextSample(); }      // Sampler::StartNextSample resets the array offsets (core/sampler.cpp:61-65)
    void SetSampleNumber(int64_t s) { array2DOffset = 0; h.SetSampleNumber(s); }
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
    const P2 *Get2DArray(int n) {        // core/sampler.cpp:93-98
        if (array2DOffset == sampleArray2D.size()) return nullptr;
        if (samples2DArraySizes[array2DOffset] != n) throw std::runtime_error("CHECK_EQ(samples2DArraySizes[array2DOffset], n) failed");
        return &sampleArray2D[array2DOffset++][(size_t)h.currentPixelSampleIndex * (size_t)n];
    }
};

struct Coverage { uint64_t nodesDeep = 0, fallbackNodes = 0, samplesDeep2 = 0; int deepest = 0; };

struct DirectLighting {
    const Renderer &r;
    int strategy, maxDepth;              // 0: UniformSampleAll, 1: UniformSampleOne
    std::vector<int> nLightSamples;
    Coverage cov;
    DirectLighting(const Renderer &r, int strategy, int maxDepth, const int32_t *nls, int nLights) : r(r), strategy(strategy), maxDepth(maxDepth) {
        if (nLights != (int)r.scene.lights.size()) throw std::runtime_error("n_lights is not the scene's");
        for (int j = 0; j < nLights; ++j) nLightSamples.push_back(nls ? nls[j] : 1);
    }
    // DirectLightingIntegrator::Preprocess, directlighting.cpp:45-60
    void Preprocess(DlSampler &sampler) const {
        if (strategy != 0) return;
        for (int i = 0; i < maxDepth; ++i)
            for (size_t j = 0; j < r.scene.lights.size(); ++j) {
                sampler.Request2DArray(nLightSamples[j]);
                sampler.Request2DArray(nLightSamples[j]);
            }
    }
    // ComputeScatteringFunctions as DirectLightingIntegrator::Li asks for it: allowMultipleLobes = false (see the head of this file)
    void Scattering(const SurfaceInteraction &isect, BSDF *bsdf) const {
        ComputeScatteringFunctions(r.scene, r.scene.materials[r.scene.shapes[isect.shape].material], isect, bsdf);
        if (bsdf->nBxDFs == 1 && bsdf->bxdfs[0].kind == BXDF_FRESNEL_SPECULAR) {      // materials/glass.cpp:62-90 with isSpecular
            const Spec R = bsdf->bxdfs[0].R, T = bsdf->bxdfs[0].S;
            const Float eta = bsdf->bxdfs[0].etaB;
            bsdf->nBxDFs = 0;
            if (!R.IsBlack()) {
                BxDF b = BxDF();
                b.kind = BXDF_SPECULAR_REFLECTION; b.type = BSDF_REFLECTION | BSDF_SPECULAR; b.R = R;
                b.frDielectric = true; b.frEtaI = 1.f; b.frEtaT = eta;
                bsdf->bxdfs[bsdf->nBxDFs++] = b;
            }
            if (!T.IsBlack()) {
                BxDF b = BxDF();
                b.kind = BXDF_SPECULAR_TRANSMISSION; b.type = BSDF_TRANSMISSION | BSDF_SPECULAR; b.R = T; b.etaA = 1.f; b.etaB = eta;
                bsdf->bxdfs[bsdf->nBxDFs++] = b;
            }
        }
    }
    // core/integrator.cpp:55-84
    Spec UniformSampleAllLights(const SurfaceInteraction &isect, const BSDF &bsdf, DlSampler &sampler, Counters &ctr) {
        Spec L(0.f);
        bool fallback = false;
        for (size_t j = 0; j < r.scene.lights.size(); ++j) {
            int nSamples = nLightSamples[j];
            const P2 *uLightArray = sampler.Get2DArray(nSamples);
            const P2 *uScatteringArray = sampler.Get2DArray(nSamples);
            if (!uLightArray || !uScatteringArray) {
                fallback = true;
                P2 uLight = sampler.Get2D();
                P2 uScattering = sampler.Get2D();
                L += r.EstimateDirect(isect, bsdf, uScattering, (int)j, uLight, ctr);
            } else {
                Spec Ld(0.f);
                for (int k = 0; k < nSamples; ++k) Ld += r.EstimateDirect(isect, bsdf, uScatteringArray[k], (int)j, uLightArray[k], ctr);
                L += Ld / nSamples;
            }
        }
        if (fallback) ++cov.fallbackNodes;
        return L;
    }
    // core/integrator.cpp:86-107 with lightDistrib == nullptr
    Spec UniformSampleOneLight(const SurfaceInteraction &isect, const BSDF &bsdf, DlSampler &sampler, Counters &ctr) {
        int nLights = (int)r.scene.lights.size();
        if (nLights == 0) return Spec(0.f);
        int lightNum = smin((int)(sampler.Get1D() * nLights), nLights - 1);
        Float lightPdf = Float(1) / nLights;
        P2 uLight = sampler.Get2D();
        P2 uScattering = sampler.Get2D();
        return r.EstimateDirect(isect, bsdf, uScattering, lightNum, uLight, ctr) / lightPdf;
    }
    // core/integrator.cpp:362-400 / 402-450.  (pdf is uninitialised in the reference and read after Sample_f's "wo.z == 0" return, which
    // leaves it untouched; 0 here and on the device.)
    Spec Specular(int type, const SurfaceInteraction &isect, const BSDF &bsdf, DlSampler &sampler, int depth, Counters &ctr) {
        V3 wo = isect.wo, wi;
        Float pdf = 0;
        Spec f = bsdf.Sample_f(wo, &wi, sampler.Get2D(), &pdf, type, nullptr);
        const V3 &ns = isect.shading.n;
        if (pdf > 0.f && !f.IsBlack() && AbsDot(wi, ns) != 0.f) {
            Ray rd = SpawnRay(isect.p, isect.pError, isect.n, wi);
            return f * Li(rd, nullptr, sampler, depth + 1, ctr) * AbsDot(wi, ns) / pdf;
        }
        return Spec(0.f);
    }
    // DirectLightingIntegrator::Li, directlighting.cpp:62-100 (every material in scope makes a BSDF: no retry of :76-81)
    Spec Li(const Ray &ray, const RayDiff *camDiff, DlSampler &sampler, int depth, Counters &ctr) {
        if (depth >= 1) ++cov.nodesDeep;
        if (depth > cov.deepest) cov.deepest = depth;
        Spec L(0.f);
        SurfaceInteraction isect;
        if (!r.SceneIntersect(ray, &isect, ctr)) {
            for (const Light &light : r.scene.lights) L += r.LightLe(light, ray.d);
            return L;
        }
        RayDiff rdiff; if (camDiff) rdiff = *camDiff;
        ComputeDifferentials(&isect, ray, rdiff);      // SurfaceInteraction::ComputeScatteringFunctions, core/interaction.cpp:93-101
        BSDF bsdf;
        Scattering(isect, &bsdf);
        V3 wo = isect.wo;
        L += r.Le(isect, wo);
        if (r.scene.lights.size() > 0) {
            if (strategy == 0) L += UniformSampleAllLights(isect, bsdf, sampler, ctr);
            else L += UniformSampleOneLight(isect, bsdf, sampler, ctr);
        }
        if (depth + 1 < maxDepth) {
            L += Specular(BSDF_REFLECTION | BSDF_SPECULAR, isect, bsdf, sampler, depth, ctr);
            L += Specular(BSDF_TRANSMISSION | BSDF_SPECULAR, isect, bsdf, sampler, depth, ctr);
        }
        return L;
    }
    // One camera sample, core/integrator.cpp:281-324 (minus the film add)
    Spec RenderSample(DlSampler &sampler, int px, int py, P2 *pFilmOut, Float *rayWeightOut, Counters &ctr) {
        P2 uf = sampler.Get2D();             // Sampler::GetCameraSample, core/sampler.cpp:46-52
        P2 pFilm((Float)px + uf.x, (Float)py + uf.y);
        Float time = sampler.Get1D(); (void)time;
        P2 pLens = sampler.Get2D();          // dimension 3: the skip test of Get2D is false (3 + 1 < arrayStartDim)
        Ray ray; RayDiff rd;
        const bool textured = !r.scene.textures.empty();
        Float rayWeight = r.camera.GenerateRay(pFilm, pLens, &ray, textured ? &rd : nullptr);
        if (textured) rd.Scale(ray, 1 / std::sqrt((Float)r.scene.prm.spp));     // core/integrator.cpp:288-289
        ++ctr.cameraRays;
        const int deepestBefore = cov.deepest;
        cov.deepest = 0;
        Spec L(0.f);
        if (rayWeight > 0) L = Li(ray, textured ? &rd : nullptr, sampler, 0, ctr);
        if (cov.deepest >= 2) ++cov.samplesDeep2;
        cov.deepest = cov.deepest > deepestBefore ? cov.deepest : deepestBefore;
        if (L.HasNaNs()) L = Spec(0.f);
        else if (L.y() < -1e-5) L = Spec(0.f);
        else if (std::isinf(L.y())) L = Spec(0.f);
        *pFilmOut = pFilm; *rayWeightOut = rayWeight;
        return L;
    }
};

void ExportCounters(const Counters &c, uint64_t *o) {      // the layout of oracle_capi.cpp's export_counters
    o[0] = c.nodesFetched; o[1] = c.nodesFetchedP; o[2] = c.nodesEntered; o[3] = c.nodesEnteredP;
    o[4] = c.triTests + c.triTestsPdf; o[5] = c.triTestsP; o[6] = c.triHits + c.triHitsPdf; o[7] = c.triHitsP;
    o[8] = c.sphereTests; o[9] = c.sphereTestsP; o[10] = c.rays; o[11] = c.shadowRays; o[12] = c.cameraRays;
}

}  // namespace

extern "C" {

const char *dlref_last_error() { return g_err.c_str(); }
void *dlref_scene_load(const char *path) {
    Renderer *r = new Renderer();
    std::string err;
    if (!LoadScene(path, &r->scene, &err) || !r->Setup(&err)) { g_err = err; delete r; return nullptr; }
    return r;
}
void dlref_scene_free(void *h) { delete (Renderer *)h; }
int dlref_n_lights(void *h) { return (int)((Renderer *)h)->scene.lights.size(); }
// Film and sampler parameters after load: crop as in the scene file (x0 x1 y0 y1 fractions); spp <= 0, center < 0: unchanged
void dlref_set_film(void *h, int xres, int yres, const float *crop4, int spp, int center) {
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
void dlref_bounds(void *h, int *out8) {
    Renderer *r = (Renderer *)h;
    out8[0] = r->film.cx0; out8[1] = r->film.cy0; out8[2] = r->film.cx1; out8[3] = r->film.cy1;
    r->film.GetSampleBounds(&out8[4], &out8[5], &out8[6], &out8[7]);
}

// SamplerIntegrator::Render (core/integrator.cpp:230-360) over tiles tileBegin, tileBegin + tileStride, ...: film_xyzw = Film::pixels
// (xyz, filterWeightSum) row-major over the cropped pixel bounds, counters13 in the oracle's layout, L3 (may be null) = the radiance of
// every camera sample after the guards, [sample][pixel of the sample bounds, row-major][3] (zero for pixels of other tiles), coverage3 =
// {nodes at depth >= 1, nodes that took the null-array fallback, camera samples with a node at depth >= 2}.  Returns 0, or -1 with
// dlref_last_error set.
int dlref_render(void *h, int strategy, int maxDepth, const int32_t *nLightSamples, int nLights, int tileBegin, int tileStride, float *film_xyzw,
                 uint64_t *counters13, float *L3, uint64_t *coverage3) try {
    Renderer *r = (Renderer *)h;
    DirectLighting dl(*r, strategy, maxDepth, nLightSamples, nLights);
    const int spp = r->scene.prm.spp;
    int sx0, sy0, sx1, sy1;
    r->film.GetSampleBounds(&sx0, &sy0, &sx1, &sy1);
    for (auto &p : r->film.pixels) p = FilmPixel();
    const int tileSize = 16;
    const int ntx = (sx1 - sx0 + tileSize - 1) / tileSize, nty = (sy1 - sy0 + tileSize - 1) / tileSize;
    const size_t nPixAll = (size_t)(sx1 - sx0) * (size_t)(sy1 - sy0);
    Counters ctr;
    DlSampler sampler(spp, sx0, sy0, sx1, sy1, r->scene.prm.samplePixelCenter != 0);
    dl.Preprocess(sampler);
    for (int t = tileBegin; t < ntx * nty; t += tileStride) {
        const int tx = t % ntx, ty = t / ntx;
        const int x0 = sx0 + tx * tileSize, x1 = smin(x0 + tileSize, sx1);
        const int y0 = sy0 + ty * tileSize, y1 = smin(y0 + tileSize, sy1);
        FilmTile tile(&r->film, x0, y0, x1, y1);
        for (int y = y0; y < y1; ++y)
            for (int x = x0; x < x1; ++x) {
                sampler.StartPixel(x, y);
                int s = 0;
                do {
                    P2 pFilm; Float w;
                    Spec L = dl.RenderSample(sampler, x, y, &pFilm, &w, ctr);
                    if (L3) {
                        float *o = L3 + 3 * ((size_t)s * nPixAll + (size_t)(y - sy0) * (size_t)(sx1 - sx0) + (size_t)(x - sx0));
                        o[0] = L.c[0]; o[1] = L.c[1]; o[2] = L.c[2];
                    }
                    tile.AddSample(pFilm, L, w);
                    ++s;
                } while (sampler.StartNextSample());
            }
        MergeFilmTile(&r->film, tile);
    }
    for (size_t i = 0; i < r->film.pixels.size(); ++i) {
        const FilmPixel &p = r->film.pixels[i];
        film_xyzw[4 * i] = p.xyz[0]; film_xyzw[4 * i + 1] = p.xyz[1]; film_xyzw[4 * i + 2] = p.xyz[2]; film_xyzw[4 * i + 3] = p.filterWeightSum;
    }
    if (counters13) ExportCounters(ctr, counters13);
    if (coverage3) { coverage3[0] = dl.cov.nodesDeep; coverage3[1] = dl.cov.fallbackNodes; coverage3[2] = dl.cov.samplesDeep2; }
    return 0;
} catch (const std::exception &e) { g_err = e.what(); return -1; }

// L of sample[i] of pixel (px[i], py[i]) after the radiance checks, taken on its own (SetSampleNumber; the arrays as StartPixel forms
// them for sample[i] + 1 samples per pixel: entry s * n + k does not depend on samplesPerPixel); L3 = 3 * n floats
int dlref_sample(void *h, int strategy, int maxDepth, const int32_t *nLightSamples, int nLights, size_t n, const int32_t *px, const int32_t *py,
                 const int64_t *sample, float *L3) try {
    Renderer *r = (Renderer *)h;
    DirectLighting dl(*r, strategy, maxDepth, nLightSamples, nLights);
    int sx0, sy0, sx1, sy1;
    r->film.GetSampleBounds(&sx0, &sy0, &sx1, &sy1);
    Counters ctr;
    for (size_t i = 0; i < n; ++i) {
        DlSampler sampler((int)sample[i] + 1, sx0, sy0, sx1, sy1, r->scene.prm.samplePixelCenter != 0);
        dl.Preprocess(sampler);
        sampler.StartPixel(px[i], py[i]);
        sampler.SetSampleNumber(sample[i]);
        P2 pFilm; Float w;
        Spec L = dl.RenderSample(sampler, px[i], py[i], &pFilm, &w, ctr);
        L3[3 * i] = L.c[0]; L3[3 * i + 1] = L.c[1]; L3[3 * i + 2] = L.c[2];
    }
    return 0;
} catch (const std::exception &e) { g_err = e.what(); return -1; }

// What the tile loop's sampler holds after Preprocess and StartPixel(px, py) with the film's samplesPerPixel: the arrays one after
// the other (u2: 2 floats per entry, array a's entry j = s * size + k), each array's size (sizes; returns their number), and per pixel
// sample the seven values GetCameraSample and one further Get2D return (cam7 = 7 * spp floats) with the dimension that Get2D read from
// (dimAfter = spp ints)
int dlref_pixel_samples(void *h, int strategy, int maxDepth, const int32_t *nLightSamples, int nLights, int px, int py, float *u2, int32_t *sizes, float *cam7,
                        int32_t *dimAfter) try {
    Renderer *r = (Renderer *)h;
    DirectLighting dl(*r, strategy, maxDepth, nLightSamples, nLights);
    int sx0, sy0, sx1, sy1;
    r->film.GetSampleBounds(&sx0, &sy0, &sx1, &sy1);
    DlSampler sampler(r->scene.prm.spp, sx0, sy0, sx1, sy1, r->scene.prm.samplePixelCenter != 0);
    dl.Preprocess(sampler);
    sampler.StartPixel(px, py);
    size_t o = 0;
    for (size_t a = 0; a < sampler.sampleArray2D.size(); ++a) {
        sizes[a] = sampler.samples2DArraySizes[a];
        for (const P2 &p : sampler.sampleArray2D[a]) { u2[o++] = p.x; u2[o++] = p.y; }
    }
    int s = 0;
    do {
        P2 a = sampler.Get2D(); Float t = sampler.Get1D(); P2 b = sampler.Get2D(); P2 c = sampler.Get2D();
        float *q = cam7 + 7 * s;
        q[0] = a.x; q[1] = a.y; q[2] = t; q[3] = b.x; q[4] = b.y; q[5] = c.x; q[6] = c.y;
        dimAfter[s] = sampler.h.dimension - 2;
        ++s;
    } while (sampler.StartNextSample());
    return (int)sampler.sampleArray2D.size();
} catch (const std::exception &e) { g_err = e.what(); return -1; }

// BSDF::Sample_f under a lobe mask (core/reflection.cpp:703-762) of shapes[shape[i]]'s material, built as DirectLightingIntegrator::Li
// builds it, at the frame frame9[9 * i ..] (n, shading.n, shading.dpdu): out8 = f (3), wi (3), pdf, 1 if some lobe matches either
// specular mask — wi and pdf preset to (9, 9, 9) and -7
int dlref_bsdf_specular(void *h, int mask, size_t n, const int32_t *shape, const float *frame9, const float *wo3, const float *u2, float *out8) {
    Renderer *r = (Renderer *)h;
    const Scene &sc = r->scene;
    DirectLighting dl(*r, 1, 1, nullptr, (int)sc.lights.size());
    for (size_t i = 0; i < n; ++i) {
        if (shape[i] < 0 || (size_t)shape[i] >= sc.shapes.size()) return -1;
        const float *fr = frame9 + 9 * i;
        SurfaceInteraction si;
        si.n = V3(fr[0], fr[1], fr[2]); si.shading.n = V3(fr[3], fr[4], fr[5]); si.shading.dpdu = V3(fr[6], fr[7], fr[8]);
        si.shape = shape[i];
        BSDF bsdf;
        dl.Scattering(si, &bsdf);
        const V3 wo(wo3[3 * i], wo3[3 * i + 1], wo3[3 * i + 2]);
        Float pdf = -7.0f; V3 w(9, 9, 9);
        const Spec f = bsdf.Sample_f(wo, &w, P2(u2[2 * i], u2[2 * i + 1]), &pdf, mask, nullptr);
        float *o = out8 + 8 * i;
        o[0] = f.c[0]; o[1] = f.c[1]; o[2] = f.c[2]; o[3] = w.x; o[4] = w.y; o[5] = w.z; o[6] = pdf;
        o[7] = bsdf.NumComponents(BSDF_REFLECTION | BSDF_SPECULAR) + bsdf.NumComponents(BSDF_TRANSMISSION | BSDF_SPECULAR) > 0 ? 1.f : 0.f;
    }
    return 0;
}

}  // extern "C"
