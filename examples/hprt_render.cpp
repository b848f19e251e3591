// hprt_render — a host program in C++ over nothing but include/hprt.h: parse (or load) a scene, build the reference's BVH,
// render it on one or several GPUs of this node and write the image.  This is the shape of the adapter a pbrt-side
// SamplerIntegrator::Render replacement has: one HprtScene per GPU, tile t of the 16x16 grid on GPU
// t mod N (core/integrator.cpp:237-244), hprt_film_gather_local as Film::MergeFilmTile, hprt_film_resolve +
// hprt_write_pfm as Film::WriteImage.  No Python, no torch: the library allocates its own device memory.
//
//   g++ -O2 -std=c++17 -pthread -Iinclude examples/hprt_render.cpp -o hprt_render -Lthesis-pbrt-v3_amd/lib -lhprt -Wl,-rpath,$PWD/thesis-pbrt-v3_amd/lib
//   ./hprt_render scene.pbrt|scene.hprt out.pfm [--spp N] [--gpus N] [--crop x0 x1 y0 y1]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "hprt.h"

#define TRY(call)                                                                                    \
    do {                                                                                             \
        int rc_ = (call);                                                                            \
        if (rc_ != HPRT_OK) { std::fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, hprt_last_error()); return 1; } \
    } while (0)

// Builds the `name` tree (hprt_<name>_build through `build`), attaches it to every scene and destroys it; 1 after printing an error.
// What the library does not walk (object instances, an unsupported "nbDirections", a tree deeper than the todo list:
// HPRT_E_UNSUPPORTED) keeps the BVH, with a warning when `warn` (a kd-tree's case is already among the model's warnings).
template <typename Tree, typename Build>
static int AttachTree(const std::string &name, Build build, int (*attach)(HprtScene *, const Tree *), void (*destroy)(Tree *),
                      const std::vector<HprtScene *> &scenes, bool warn) {
    Tree *t = nullptr;
    const int rc = build(&t);
    if (rc == HPRT_E_UNSUPPORTED) {
        if (warn) std::fprintf(stderr, "Warning: %s; \"bvh\" used\n", hprt_last_error());
        return 0;
    }
    if (rc != HPRT_OK) { std::fprintf(stderr, "hprt_%s_build failed (%d): %s\n", name.c_str(), rc, hprt_last_error()); return 1; }
    int arc = HPRT_OK;
    for (size_t g = 0; g < scenes.size() && arc == HPRT_OK; ++g) arc = attach(scenes[g], t);
    destroy(t);
    if (arc != HPRT_OK) { std::fprintf(stderr, "hprt_scene_attach_%s failed (%d): %s\n", name.c_str(), arc, hprt_last_error()); return 1; }
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s scene.pbrt|scene.hprt out.pfm [--spp N] [--gpus N] [--crop x0 x1 y0 y1]\n", argv[0]); return 2; }
    const std::string scenePath = argv[1], outPath = argv[2];
    int spp = 0, gpus = 1;
    float crop[4] = {0, 1, 0, 1}; bool haveCrop = false;
    for (int i = 3; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--spp") && i + 1 < argc) spp = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--gpus") && i + 1 < argc) gpus = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--crop") && i + 4 < argc) { for (int k = 0; k < 4; ++k) crop[k] = (float)std::atof(argv[++i]); haveCrop = true; }
        else { std::fprintf(stderr, "unknown argument %s\n", argv[i]); return 2; }
    }
    if (gpus < 1) gpus = 1;

    // pbrtParseFile / the baked container (core/api.cpp, csrc/scene_io.cpp)
    HprtModel *model = nullptr;
    const bool baked = scenePath.size() > 5 && scenePath.substr(scenePath.size() - 5) == ".hprt";
    if (baked) TRY(hprt_model_load(scenePath.c_str(), &model));
    else TRY(hprt_model_parse(scenePath.c_str(), nullptr, 0, &model));
    if (const char *w = hprt_model_warnings(model)) if (*w) std::fprintf(stderr, "%s\n", w);
    HprtRenderOptions opt;
    TRY(hprt_model_get_options(model, &opt));
    if (spp > 0) opt.spp = spp;
    if (haveCrop) std::memcpy(opt.crop, crop, sizeof(crop));

    char accel[64] = "";
    TRY(hprt_model_accelerator(model, accel, sizeof(accel)));
    const std::string acc = accel;
    // Integrator "ambientocclusion" (core/api.cpp:1922): hprt_render_ao with the directive's "nsamples" and "cossample"; every other name
    // renders the path integrator.  (The cross-tile film records a multi-GPU gather merges stay with hprt_render.)
    char integ[64] = "";
    HprtAoParams ao;
    TRY(hprt_model_integrator(model, integ, sizeof(integ), &ao));
    const bool ambientOcclusion = std::string(integ) == "ambientocclusion";
    if (ambientOcclusion && gpus > 1) { std::fprintf(stderr, "Integrator \"ambientocclusion\" renders on one GPU (--gpus 1)\n"); return 2; }
    // Integrator "directlighting" (core/api.cpp:1913): hprt_render_direct with the directive's "strategy" and "maxdepth" and every light's
    // sample count as the scene file gives it
    const bool directLighting = std::string(integ) == "directlighting";
    HprtDirectParams direct;
    size_t nLights = 0;
    TRY(hprt_model_direct(model, &direct, nullptr, 0, &nLights));
    std::vector<int32_t> lightSamples(nLights, 1);
    if (nLights) TRY(hprt_model_direct(model, nullptr, lightSamples.data(), nLights, nullptr));
    if (directLighting && gpus > 1) { std::fprintf(stderr, "Integrator \"directlighting\" renders on one GPU (--gpus 1)\n"); return 2; }
    const char *renderName = ambientOcclusion ? "hprt_render_ao" : directLighting ? "hprt_render_direct" : "hprt_render";

    // BVHAccel's constructor on the host (accelerators/bvh.cpp:181-250); for Accelerator "bvhold" BVHAccelOld's
    // (accelerators/bvhOld.cpp:185-227) with the Accelerator line's split method: the same handle, the same walks
    HprtBvh *bvh = nullptr;
    if (acc == "bvhold") TRY(hprt_bvhold_build(model, nullptr, &bvh));
    else TRY(hprt_bvh_build(model, &bvh));

    // croppedPixelBounds (core/film.cpp:56-60)
    const int x0 = (int)std::ceil((float)opt.xres * opt.crop[0]), x1 = (int)std::ceil((float)opt.xres * opt.crop[1]);
    const int y0 = (int)std::ceil((float)opt.yres * opt.crop[2]), y1 = (int)std::ceil((float)opt.yres * opt.crop[3]);
    const int W = x1 - x0, H = y1 - y0;
    if (W <= 0 || H <= 0) { std::fprintf(stderr, "empty film\n"); return 1; }
    const size_t nPix = (size_t)W * (size_t)H;

    // one scene per GPU; rank r renders tiles r, r + N, ...
    std::vector<HprtScene *> scenes((size_t)gpus, nullptr);
    for (int g = 0; g < gpus; ++g) TRY(hprt_scene_create_from_model(model, bvh, g, &scenes[(size_t)g]));
    // Accelerator "kdtree", "rbsp", "rbspkd", "bsppaper", "bsppaperkd" or a node-based BSP tree (MakeAccelerator, core/api.cpp:790-831): the tree is built on the host from the
    // scene's Accelerator line and every scene walks it
    int arc = 0;
    if (acc == "kdtree") arc = AttachTree<HprtKdTree>(acc, [&](HprtKdTree **t) { return hprt_kdtree_build(model, t); }, hprt_scene_attach_kdtree, hprt_kdtree_destroy, scenes, false);
    if (acc == "rbsp") arc = AttachTree<HprtRbsp>(acc, [&](HprtRbsp **t) { return hprt_rbsp_build(model, nullptr, t); }, hprt_scene_attach_rbsp, hprt_rbsp_destroy, scenes, true);
    if (acc == "rbspkd") arc = AttachTree<HprtRbspKd>(acc, [&](HprtRbspKd **t) { return hprt_rbspkd_build(model, nullptr, t); }, hprt_scene_attach_rbspkd, hprt_rbspkd_destroy, scenes, true);
    if (acc == "bsppaper") arc = AttachTree<HprtBspPaper>(acc, [&](HprtBspPaper **t) { return hprt_bsppaper_build(model, nullptr, t); }, hprt_scene_attach_bsppaper, hprt_bsppaper_destroy, scenes, true);
    if (acc == "bsppaperkd") arc = AttachTree<HprtBspPaperKd>(acc, [&](HprtBspPaperKd **t) { return hprt_bsppaperkd_build(model, nullptr, t); }, hprt_scene_attach_bsppaperkd, hprt_bsppaperkd_destroy, scenes, true);
    // the node-based BSP trees ("bspcluster", "bsprandomwithkd", "bsparbitraryfastkd", ...: Create...TreeAccelerator of
    // accelerators/bsp{Arbitrary,Cluster,Random}{,WithKd,FastKd}.cpp): a fastkd tree is a bsppaperkd tree, the others bsppaper trees
    const bool nodeBased = acc.rfind("bsparbitrary", 0) == 0 || acc.rfind("bspcluster", 0) == 0 || acc.rfind("bsprandom", 0) == 0;
    const bool fastKd = acc.size() > 6 && acc.compare(acc.size() - 6, 6, "fastkd") == 0;
    if (nodeBased && fastKd) arc = AttachTree<HprtBspPaperKd>(acc, [&](HprtBspPaperKd **t) { return hprt_bspnodekd_build(model, nullptr, t); }, hprt_scene_attach_bsppaperkd, hprt_bsppaperkd_destroy, scenes, true);
    if (nodeBased && !fastKd) arc = AttachTree<HprtBspPaper>(acc, [&](HprtBspPaper **t) { return hprt_bspnode_build(model, nullptr, t); }, hprt_scene_attach_bsppaper, hprt_bsppaper_destroy, scenes, true);
    if (arc) return 1;
    // one host thread per GPU (the renders are independent; errors are thread-local in the library, so each thread keeps its own)
    std::vector<HprtRenderStats> stats((size_t)gpus);
    std::vector<int> rcs((size_t)gpus, HPRT_OK);
    std::vector<std::string> errs((size_t)gpus);
    std::vector<std::thread> workers;
    for (int g = 0; g < gpus; ++g)
        workers.emplace_back([&, g] {
            HprtRenderDesc desc; std::memset(&desc, 0, sizeof(desc));
            desc.opt = opt; desc.tile_begin = g; desc.tile_end = 0; desc.tile_stride = gpus;
            desc.flags = gpus > 1 ? HPRT_RENDER_EXPORT_FOREIGN : 0;
            // (the library-owned film of this scene)
            rcs[(size_t)g] = ambientOcclusion ? hprt_render_ao(scenes[(size_t)g], &desc, &ao, nullptr, nullptr, &stats[(size_t)g])
                             : directLighting ? hprt_render_direct(scenes[(size_t)g], &desc, &direct, lightSamples.data(), nLights, nullptr, nullptr, &stats[(size_t)g])
                                              : hprt_render(scenes[(size_t)g], &desc, nullptr, nullptr, &stats[(size_t)g]);
            if (rcs[(size_t)g] != HPRT_OK) errs[(size_t)g] = hprt_last_error();
        });
    for (std::thread &t : workers) t.join();
    HprtRenderStats total; std::memset(&total, 0, sizeof(total));
    double seconds = 0;
    for (int g = 0; g < gpus; ++g) {
        if (rcs[(size_t)g] != HPRT_OK) { std::fprintf(stderr, "%s on GPU %d failed (%d): %s\n", renderName, g, rcs[(size_t)g], errs[(size_t)g].c_str()); return 1; }
        const HprtRenderStats &st = stats[(size_t)g];
        total.camera_rays += st.camera_rays; total.rays += st.rays; total.shadow_rays += st.shadow_rays;
        if (st.render_seconds > seconds) seconds = st.render_seconds;
    }
    if (gpus > 1) TRY(hprt_film_gather_local(scenes.data(), nullptr, gpus, nPix, 0));      // Film::MergeFilmTile across GPUs (RCCL)

    // Film::WriteImage (core/film.cpp:266-303)
    std::vector<float> xyzw(4 * nPix), rgb(3 * nPix);
    TRY(hprt_film_read(scenes[0], xyzw.data(), nPix));
    TRY(hprt_film_resolve(xyzw.data(), nPix, opt.film_scale, rgb.data()));
    TRY(hprt_write_pfm(outPath.c_str(), rgb.data(), W, H));
    std::printf("%s: %dx%d, %d spp on %d GPU(s): %.3f s, %.1f Mrays/s (%llu camera + %llu path + %llu shadow rays) -> %s\n", hprt_version(), W, H,
                opt.spp, gpus, seconds, seconds > 0 ? (double)(total.rays + total.shadow_rays) / seconds * 1e-6 : 0.0,
                (unsigned long long)total.camera_rays, (unsigned long long)total.rays, (unsigned long long)total.shadow_rays, outPath.c_str());
    for (HprtScene *s : scenes) hprt_scene_destroy(s);
    hprt_bvh_destroy(bvh);
    hprt_model_destroy(model);
    return 0;
}
