/* hprt — C ABI of the MI355X-native wavefront path-tracing core.
 *
 * Drop-in boundary for ONE hot path of the pbrt-v3 thesis fork
 * (jhoobergs/Thesis-pbrt-v3):
 *   SamplerIntegrator::Render  ->  PathIntegrator::Li  ->
 *   BVHAccel::Intersect/IntersectP  ->  Triangle::Intersect/IntersectP.
 * Plain pointers and sizes only; no C++ or torch types cross this header.
 * Every entry point names the reference interface it stands in for
 * (paths relative to the reference's src/).  All functions return 0 on success
 * or a negative HPRT_E_* code; hprt_last_error() returns the message of the last
 * failure on the calling thread.  No exception crosses the boundary.
 *
 * Device entry points (hprt_scene_*, hprt_intersect, hprt_occluded, hprt_render,
 * hprt_film_*) require a gfx950 GPU and fail with HPRT_E_NO_DEVICE otherwise:
 * there is no CPU fallback behind this ABI.  hprt_scene_create checks the scene
 * description first: a malformed one is reported as such (HPRT_E_INVALID or
 * HPRT_E_UNSUPPORTED) even without a device.
 *
 * Concurrency.  An HprtScene allows ONE call in flight at a time: its work counter,
 * ray / hit staging, traversal-stack area and render workspace belong to the scene,
 * not to a call.  The library enforces it — calls from several host threads take the
 * scene's mutex, and a call on one HIP stream first waits (on the device) for an
 * earlier asynchronous *_device call on another — so concurrent use is SAFE but
 * serialised: where pbrt calls BVHAccel::Intersect from every worker thread
 * (core/parallel.cpp:247-299), a host gains nothing by doing the same here; it should
 * batch.  HprtModel / HprtBvh objects are immutable after creation and may be read
 * from any number of threads.  Different HprtScene objects are independent.
 */
#ifndef HPRT_H
#define HPRT_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define HPRT_OK 0
#define HPRT_E_INVALID (-1)     /* bad argument / malformed description */
#define HPRT_E_IO (-2)          /* file could not be read or written     */
#define HPRT_E_PARSE (-3)       /* scene description rejected            */
#define HPRT_E_NO_DEVICE (-4)   /* no usable HIP device                  */
#define HPRT_E_DEVICE (-5)      /* HIP runtime error                     */
#define HPRT_E_UNSUPPORTED (-6) /* feature outside the hot-path scope    */

const char *hprt_last_error(void);
/* Compile-time identity of the library: "hprt <ver> gfx950 ..." */
const char *hprt_version(void);

/* ------------------------------------------------------------------------ */
/* Host front-end: the parsed scene ("model").                               */
/* Stands in for pbrtParseFile + the pbrt* API state machine                 */
/* (core/parser.cpp:786-1092, core/api.cpp:1103-1874) up to, but excluding,  */
/* MakeScene()/Render().                                                     */
/* ------------------------------------------------------------------------ */
typedef struct HprtModel HprtModel;

typedef struct HprtRenderOptions {
    int32_t xres, yres;            /* Film "xresolution"/"yresolution" (core/film.cpp:322-323) */
    float crop[4];                 /* cropwindow x0 x1 y0 y1 (core/film.cpp:326-341)           */
    float filter_radius[2];        /* box filter half-widths (filters/box.cpp:43-47)            */
    float film_scale, max_sample_luminance;
    float fov, lens_radius, focal_distance;      /* cameras/perspective.cpp:224-271 */
    float screen_window[4];        /* x0 x1 y0 y1 */
    float camera_to_world[16], world_to_camera[16]; /* row-major Transform::m / mInv */
    int32_t spp;                   /* Sampler "pixelsamples" (samplers/halton.cpp:135)          */
    int32_t sample_pixel_center;
    int32_t max_depth;             /* Integrator "maxdepth" (integrators/path.cpp:209)          */
    float rr_threshold;            /* integrators/path.cpp:224                                   */
    int32_t light_strategy;        /* 0 uniform, 1 power, 2 spatial (core/lightdistrib.cpp:47-66); all three built */
    int32_t max_node_prims, isect_cost, trav_cost; /* accelerators/bvh.cpp:529-535 */
} HprtRenderOptions;

/* Parse a .pbrt file.  `subst` holds n_subst {key,value} string pairs that
 * replace the fork's template tokens ($acc -> "bvh", $accnr -> 0, ... as
 * scripts/render_simple.sh:23-29 does with sed) and, for keys that end in '/',
 * path prefixes of Include/plymesh file names. */
int hprt_model_parse(const char *pbrt_path, const char *const *subst, int n_subst, HprtModel **out);
/* Image textures of a parsed model (built MIPMaps): count[0] = textures; info = {levels, trilinear, wrap, width
 * and height of level 0}; hprt_model_texture_level copies 3*w*h floats of one level (rgb may be NULL to query w,h). */
int hprt_model_texture_info(const HprtModel *m, uint32_t texture, int32_t info[5], float *max_anisotropy);
int hprt_model_texture_level(const HprtModel *m, uint32_t texture, uint32_t level, int32_t wh[2], float *rgb);
/* Baked scene container (post-parse, world-space; DESIGN.md "Baked scene"). */
int hprt_model_load(const char *baked_path, HprtModel **out);
int hprt_model_save(const HprtModel *m, const char *baked_path);
/* The same with every image texture stored as the image it was read from (8-bit texels as the file held them + the
 * conversion parameters of ImageTexture::GetTexture, textures/imagemap.cpp:52-97) instead of its finished float pyramid:
 * 3 bytes per source texel instead of 16 per power-of-two texel.  hprt_model_load rebuilds the pyramid with the MIPMap
 * constructor that built it at parse time (core/mipmap.h:113-201), so both forms load to the same floats. */
int hprt_model_save_compact(const HprtModel *m, const char *baked_path);
void hprt_model_destroy(HprtModel *m);
int hprt_model_get_options(const HprtModel *m, HprtRenderOptions *out);
int hprt_model_set_options(HprtModel *m, const HprtRenderOptions *in);
/* counts[0..6] = shapes, primitives, triangles, spheres, materials, lights, image textures */
int hprt_model_counts(const HprtModel *m, uint64_t counts[7]);
/* Front-end warnings (out-of-scope features that were substituted), '\n' separated. */
const char *hprt_model_warnings(const HprtModel *m);

/* ------------------------------------------------------------------------ */
/* Accelerator build.  Stands in for BVHAccel::BVHAccel + iterativeBuild +   */
/* flattenBVHTree (accelerators/bvh.cpp:155-185, 196-333, 335-350) and       */
/* CreateBVHAccelerator (:529-535).  Host side; the node array is            */
/* byte-identical to the reference's LinearBVHNode[] (:123-152).             */
/* ------------------------------------------------------------------------ */
typedef struct HprtBvh HprtBvh;
int hprt_bvh_build(const HprtModel *m, HprtBvh **out);
/* The same from the primitives' world bounds (Primitive::WorldBound(), core/primitive.h:55):
 * bmin/bmax hold 3 floats per primitive in creation order. */
int hprt_bvh_build_from_bounds(size_t n_prims, const float *bmin, const float *bmax, int max_node_prims, int isect_cost,
                               int trav_cost, HprtBvh **out);
void hprt_bvh_destroy(HprtBvh *b);
/* info[0..3] = nodes, primitives, leaves, max depth; bounds6 = root pMin,pMax
 * (BVHAccel::WorldBound, accelerators/bvh.cpp:187-189) */
int hprt_bvh_info(const HprtBvh *b, uint32_t info[4], float bounds6[6]);
/* nodes32: n_nodes*32 bytes; prim_order: n_prims uint32 (ordered -> creation number) */
int hprt_bvh_copy(const HprtBvh *b, void *nodes32, uint32_t *prim_order);
/* The same for the aggregate of object definition `object` (core/api.cpp:1798-1806). */
int hprt_bvh_object_info(const HprtBvh *b, uint32_t object, uint32_t info[4], float bounds6[6]);
int hprt_bvh_object_copy(const HprtBvh *b, uint32_t object, void *nodes32, uint32_t *prim_order);

/* ------------------------------------------------------------------------ */
/* Accelerator "bvhold": the stock pbrt-v3 BVH the fork keeps as            */
/* BVHAccelOld.  Stands in for BVHAccelOld::BVHAccelOld                      */
/* (accelerators/bvhOld.cpp:185-227), recursiveBuild (:238-404), HLBVHBuild / */
/* emitLBVH / buildUpperSAH (:406-640), flattenBVHTree (:642-660) and        */
/* CreateBVHAcceleratorOld (:742-762).  The result is an ordinary HprtBvh:   */
/* hprt_bvh_info / _copy, their object variants, hprt_bvh_destroy and        */
/* hprt_scene_create_from_model take it unchanged, and the walks walk it as  */
/* they walk the fork's tree (BVHAccelOld::Intersect / IntersectP, :664-740, */
/* are BVHAccel's).  An interior node's count is 0 (LinearBVHNodeOld).       */
/* Models with object instances: every object of more than one primitive    */
/* gets a tree with the same parameters (pbrtObjectInstance,                 */
/* core/api.cpp:1798-1806), the top level is built over                      */
/* TransformedPrimitive::WorldBound.  HPRT_E_UNSUPPORTED where the           */
/* reference's build is undefined: the CHECK_NE of :566 (hlbvh: the treelet  */
/* roots' centroids coincide on the widest axis), bounds that are not        */
/* finite, a centroid outside the 12 SAH buckets (:331-332, :585-586: bounds */
/* whose sum overflows), a leaf of 65,536 primitives or more (:648), more    */
/* than 2^31 - 1 primitives (the device entries: more than 2^26 per tree,    */
/* what their one-workgroup scan serves).  A leaf of more than 255 primitives (coincident      */
/* codes, a degenerate centroid extent) is laid out and walked like any      */
/* other: the layout marks a leaf's last primitive and keeps no count.       */
/* ------------------------------------------------------------------------ */
enum { HPRT_BVHOLD_SAH = 0, HPRT_BVHOLD_HLBVH = 1, HPRT_BVHOLD_MIDDLE = 2, HPRT_BVHOLD_EQUAL = 3 };
typedef struct HprtBvhOldParams {
    int32_t split_method;     /* HPRT_BVHOLD_*: "string splitmethod" sah | hlbvh | middle | equal (:744-758) */
    int32_t max_node_prims;   /* "integer maxnodeprims" (:760); min(255, .) applies (:187) */
} HprtBvhOldParams;
/* params NULL: the parameters of the model's Accelerator line (defaults sah, 4) */
int hprt_bvhold_build(const HprtModel *m, const HprtBvhOldParams *params, HprtBvh **out);
/* The same from the primitives' world bounds (3 floats per primitive, creation order); params NULL: sah, 4 */
int hprt_bvhold_build_from_bounds(size_t n_prims, const float *bmin, const float *bmax, const HprtBvhOldParams *params, HprtBvh **out);
/* The HLBVH form built on the GPU (opt-in): HLBVHBuild's centroid bounds, Morton codes (:415-424), radix sort (:141-182),
 * treelet intervals (:431-449) and emitLBVH (:476-538) run as gfx950 kernels; buildUpperSAH (:540-640) over the at most
 * 4,096 treelet roots and the final depth-first array stay on the host.  Returns the same bytes as hprt_bvhold_build with
 * split_method HPRT_BVHOLD_HLBVH.  A treelet of more than serial_treelet_max primitives is emitted on the host from the
 * downloaded sorted array.  Another split method: HPRT_E_UNSUPPORTED (hprt_bvhold_build builds it).  Without a HIP device:
 * HPRT_E_NO_DEVICE and *out stays NULL.  Models with object instances: every tree goes through the one device session. */
typedef struct HprtBvhOldDeviceOpts {
    int device;                    /* HIP device ordinal */
    uint32_t serial_treelet_max;   /* largest treelet one lane emits; 0 = default (4096) */
} HprtBvhOldDeviceOpts;
typedef struct HprtBvhOldDeviceStats {
    uint64_t prims_sorted, sort_passes, treelets, treelets_host, launches;   /* summed over the model's trees */
    double seconds_device;         /* wall time of the device steps, staging and downloads included */
} HprtBvhOldDeviceStats;
/* opts NULL: device 0 and the defaults; stats may be NULL */
int hprt_bvhold_build_device(const HprtModel *m, const HprtBvhOldParams *params, const HprtBvhOldDeviceOpts *opts, HprtBvhOldDeviceStats *stats,
                             HprtBvh **out);
int hprt_bvhold_build_device_from_bounds(size_t n_prims, const float *bmin, const float *bmax, const HprtBvhOldParams *params,
                                         const HprtBvhOldDeviceOpts *opts, HprtBvhOldDeviceStats *stats, HprtBvh **out);

/* ------------------------------------------------------------------------ */
/* kd-tree (Accelerator "kdtree").  Stands in for KdTreeAccel::KdTreeAccel +  */
/* buildTree (accelerators/kdtreeaccel.cpp:163-380) and                       */
/* CreateKdTreeAccelerator (:523-545).  Host side; the node array is          */
/* byte-identical to the reference's KdAccelNode[] (8 bytes per node: split   */
/* or onePrimitive or primitiveIndicesOffset, then flags | nPrims << 2 or     */
/* axis | aboveChild << 2) and primitiveIndices; primitives are numbered in   */
/* creation order.  splitalpha / alphatype / axisselectiontype /              */
/* axisselectionamount only feed the reference's statistics and are ignored.  */
/* ------------------------------------------------------------------------ */
typedef struct HprtKdTree HprtKdTree;
/* The scene's Accelerator name as written ("bvh", "kdtree", ...): cap bytes including the terminating 0.  Baked models
 * report "bvh". */
int hprt_model_accelerator(const HprtModel *m, char *name, size_t cap);
/* CreateAOIntegrator's parameters (integrators/ao.cpp:105-126): "nsamples" 64, "cossample" true */
typedef struct HprtAoParams { int32_t n_samples; int32_t cos_sample; } HprtAoParams;
/* The scene's Integrator name as written ("path", "ambientocclusion", ...): cap bytes including the terminating 0; ao (may
 * be NULL) receives the parameters of an Integrator "ambientocclusion" line, the defaults for every other name.  Like the
 * accelerators' parameters these live on the host side of the model and are not baked: baked models report "path". */
int hprt_model_integrator(const HprtModel *m, char *name, size_t cap, HprtAoParams *ao);
/* CreateDirectLightingIntegrator's parameters (integrators/directlighting.cpp:102-135): "strategy" "all" (0) or "one"
 * (1), "maxdepth" 5 */
typedef struct HprtDirectParams { int32_t strategy; /* 0 all, 1 one */ int32_t max_depth; } HprtDirectParams;
/* hprt_render_direct refuses a max_depth above this (HPRT_E_UNSUPPORTED) */
#define HPRT_DIRECT_MAX_DEPTH 8
/* The parameters of the scene's Integrator "directlighting" line (the defaults, all and 5, for every other name), and
 * Light::nSamples of every scene light in scene.lights order — one entry per triangle of a mesh emitter — as
 * UniformSampleAllLights reads it: max(1, "samples" or else "nsamples") of AreaLightSource "diffuse" and LightSource
 * "infinite" (lights/diffuse.cpp:140-141, lights/infinite.cpp:181-182, core/light.cpp:45), 1 for "point" and "distant".
 * params and n_light_samples may be NULL; *n_lights (may be NULL) receives the number of lights, of which the first
 * min(cap, *n_lights) are written.  Host side of the model, not baked: baked models report the defaults and 1. */
int hprt_model_direct(const HprtModel *m, HprtDirectParams *params, int32_t *n_light_samples, size_t cap, size_t *n_lights);
/* Built with the parameters of the scene's Accelerator line (defaults intersectcost 80, traversalcost 1, emptybonus 0,
 * maxprims 1, maxdepth -1 = round(2 + 1.6 Log2Int(N))).  Models with object instances: HPRT_E_UNSUPPORTED. */
int hprt_kdtree_build(const HprtModel *m, HprtKdTree **out);
/* The same from the primitives' world bounds (3 floats per primitive, creation order). */
int hprt_kdtree_build_from_bounds(size_t n_prims, const float *bmin, const float *bmax, int isect_cost, int trav_cost,
                                  float empty_bonus, int max_prims, int max_depth, HprtKdTree **out);
/* info[0..3] = nodes, leaves, primitive references (primitiveIndices entries), depth (interior levels of the deepest
 * path).  A tree deeper than HPRT_KD_MAX_DEPTH is refused by the builders with HPRT_E_UNSUPPORTED. */
int hprt_kdtree_info(const HprtKdTree *t, uint32_t info[4]);
#define HPRT_KD_MAX_DEPTH 64       /* the device walk's todo capacity: pbrt's maxTodo (kdtreeaccel.cpp:393) */
/* nodes8: info[0] * 8 bytes; prim_indices: info[2] uint32 (either may be NULL) */
int hprt_kdtree_copy(const HprtKdTree *t, void *nodes8, uint32_t *prim_indices);
void hprt_kdtree_destroy(HprtKdTree *t);

/* ------------------------------------------------------------------------ */
/* Two-level kd-trees (Accelerator "kdtree" on a model with object           */
/* instances).  Stands in for pbrtObjectInstance (core/api.cpp:1794-1819):   */
/* MakeAccelerator(renderOptions->AcceleratorName, ...) over the primitives  */
/* of every object that has more than one (an object with exactly one is     */
/* wrapped as it is, :1798), each wrapped in a TransformedPrimitive, and     */
/* pbrtWorldEnd's top-level accelerator over those wrappers: a kd-tree whose */
/* leaves hold kd-trees.  Opt-in: hprt_kdtree_build keeps refusing such      */
/* models and the front end keeps their BVH and its warning.                 */
/* ------------------------------------------------------------------------ */
typedef struct HprtKdInst HprtKdInst;
/* One KdTreeAccel per object with more than one primitive, over the object's primitive bounds in object space, and the
 * top-level KdTreeAccel over the top-level items in creation order; an instance is bounded by
 * TransformedPrimitive::WorldBound (core/primitive.h:116-118).  Every tree takes the parameters of the scene's Accelerator
 * line; maxdepth -1 resolves per tree from its own primitive count, as in hprt_kdtree_build.
 * HPRT_E_UNSUPPORTED for a model without instances (hprt_kdtree_build's job) and when depth(top) + deepest object depth + 1
 * exceeds HPRT_KD_MAX_DEPTH: the walk keeps both levels' todo entries and one saved top-level position in one list. */
int hprt_kdinst_build(const HprtModel *m, HprtKdInst **out);
/* info[0..3] = nodes, leaves, primitive references, depth of the top-level tree; info[4] = object definitions, info[5] =
 * object trees (objects with more than one primitive), info[6] = the deepest object tree's depth, info[7] = instances. */
int hprt_kdinst_info(const HprtKdInst *t, uint32_t info[8]);
/* info[0..3] as hprt_kdtree_info for the tree of object definition `object`; all zero for an object of one primitive,
 * which has no tree (core/api.cpp:1798). */
int hprt_kdinst_object_info(const HprtKdInst *t, uint32_t object, uint32_t info[4]);
/* The arrays of the top-level tree / of one object's tree, as hprt_kdtree_copy returns them (either may be NULL). */
int hprt_kdinst_copy(const HprtKdInst *t, void *nodes8, uint32_t *prim_indices);
int hprt_kdinst_object_copy(const HprtKdInst *t, uint32_t object, void *nodes8, uint32_t *prim_indices);
void hprt_kdinst_destroy(HprtKdInst *t);

/* ------------------------------------------------------------------------ */
/* RBSP tree (Accelerator "rbsp").  Stands in for RBSP::buildTree           */
/* (accelerators/rbsp.cpp:181-403): a kd-tree whose split planes may also   */
/* be oblique, chosen from M = 3, 7, 9 or 13 fixed directions, with the     */
/* node's k-DOP as the surface of the cost model.  Byte-identical to the    */
/* reference: 8-byte RBSPNode[] (word 0 split / onePrimitive /              */
/* primitiveIndicesOffset; word 1 flags: leaf M | nPrims << off, interior   */
/* axis | aboveChild << off, off = 32 - clz(M)), primitiveIndices and the   */
/* direction table.  splitalpha, alphatype, axisselectiontype and           */
/* axisselectionamount are never read by buildTree and are ignored.         */
/* ------------------------------------------------------------------------ */
typedef struct HprtRbsp HprtRbsp;
typedef struct HprtRbspParams {
    int isect_cost;     /* "intersectcost", default 80 */
    int trav_cost;      /* "traversalcost", default 5 */
    float empty_bonus;  /* "emptybonus", default 0 */
    int max_prims;      /* "maxprims", default 1 */
    int max_depth;      /* "maxdepth", default -1 = round(2 + 1.6 Log2Int(N)) */
    int n_directions;   /* "nbDirections": 3 (default), 7, 9 or 13; anything else is HPRT_E_UNSUPPORTED */
    int threads;        /* builder threads (0: OMP_NUM_THREADS, else 16; at most 16); the tree does not depend on it */
} HprtRbspParams;
/* params NULL: the scene's Accelerator line (baked models report "bvh" and get the defaults).  Models with object
 * instances: HPRT_E_UNSUPPORTED (their two-level trees are opt-in: hprt_rbspinst_build).  A tree deeper than HPRT_RBSP_MAX_DEPTH: HPRT_E_UNSUPPORTED. */
int hprt_rbsp_build(const HprtModel *m, const HprtRbspParams *params, HprtRbsp **out);
/* The same over n triangles (9 floats each: three world-space vertices, creation order); params NULL: the defaults. */
int hprt_rbsp_build_from_triangles(size_t n_tris, const float *p9, const HprtRbspParams *params, HprtRbsp **out);
/* info[0..4] = nodes, leaves, primitive references (primitiveIndices entries), depth (interior levels of the deepest
 * path), M (directions) */
int hprt_rbsp_info(const HprtRbsp *t, uint32_t info[5]);
#define HPRT_RBSP_MAX_DEPTH 64     /* the device walk's todo capacity: pbrt's maxTodo (rbsp.cpp:416) */
/* nodes8: info[0] * 8 bytes; prim_indices: info[2] uint32; directions: 3 * M floats (any may be NULL) */
int hprt_rbsp_copy(const HprtRbsp *t, void *nodes8, uint32_t *prim_indices, float *directions);
void hprt_rbsp_destroy(HprtRbsp *t);

/* ------------------------------------------------------------------------ */
/* kd-aware RBSP tree (Accelerator "rbspkd").  Stands in for                */
/* RBSPKd::buildTree (accelerators/rbspKd.cpp:194-488): the RBSP tree's     */
/* node layout, directions and k-DOP cost model, with axis splits costed    */
/* kd_trav_cost + C_isect and oblique ones                                  */
/* 0.1 * isect_cost * (N - 1) + kd_trav_cost + C_isect (a second minimum,   */
/* trav_cost + C_isect over the oblique splits, takes part in the leaf      */
/* tests only).  A handle of its own: an rbspkd tree is walked with the kd  */
/* form at axis nodes and can never be attached to the RBSP walk.           */
/* ------------------------------------------------------------------------ */
typedef struct HprtRbspKd HprtRbspKd;
typedef struct HprtRbspKdParams {
    int isect_cost;     /* "intersectcost", default 80 */
    int trav_cost;      /* "traversalcost", default 5 */
    int kd_trav_cost;   /* "kdtraversalcost", default 1 */
    float empty_bonus;  /* "emptybonus", default 0 */
    int max_prims;      /* "maxprims", default 1 */
    int max_depth;      /* "maxdepth", default -1 = round(2 + 1.6 Log2Int(N)) */
    int n_directions;   /* "nbDirections": 3 (default), 7, 9 or 13; anything else is HPRT_E_UNSUPPORTED */
    int threads;        /* builder threads (0: OMP_NUM_THREADS, else 16; at most 16); the tree does not depend on it */
} HprtRbspKdParams;
/* As hprt_rbsp_build: params NULL takes the scene's Accelerator line; instanced models, an unsupported M and trees deeper than
 * HPRT_RBSP_MAX_DEPTH are HPRT_E_UNSUPPORTED, and so is a node where only the fixed-cost minimum is finite (the reference's
 * build reads edges[-1] there). */
int hprt_rbspkd_build(const HprtModel *m, const HprtRbspKdParams *params, HprtRbspKd **out);
int hprt_rbspkd_build_from_triangles(size_t n_tris, const float *p9, const HprtRbspKdParams *params, HprtRbspKd **out);
/* info[0..6] = nodes, leaves, primitive references, depth, M, kd interior nodes (direction < 3), oblique interior nodes */
int hprt_rbspkd_info(const HprtRbspKd *t, uint32_t info[7]);
int hprt_rbspkd_copy(const HprtRbspKd *t, void *nodes8, uint32_t *prim_indices, float *directions);
void hprt_rbspkd_destroy(HprtRbspKd *t);

/* ------------------------------------------------------------------------ */
/* Device-assisted builds of the two RBSP trees (opt-in).  They stand in    */
/* for the same RBSP::buildTree / RBSPKd::buildTree and return the same     */
/* bytes as hprt_rbsp_build / hprt_rbspkd_build: the tree logic (sorts, the */
/* first-minimum scan, leaf tests, the winner's cut, classification) stays  */
/* on the host; what moves to the GPU is the costing of a node's split      */
/* candidates (KDOPCut + KDOPSurfaceArea of accelerators/kDOPMesh.h and the */
/* cost formulas of rbsp.cpp:262-283 / rbspKd.cpp:283-318), one candidate   */
/* per lane, for nodes with at least min_candidates candidates.  A          */
/* candidate whose half-meshes outgrow the kernel's fixed capacity is       */
/* costed again on the host.  Same handles: info, copy, attach and the      */
/* walks are unchanged.  Refusals are those of the host entries; without a  */
/* HIP device: HPRT_E_NO_DEVICE and *out stays NULL.                        */
/* ------------------------------------------------------------------------ */
typedef struct HprtBuildDeviceOpts {
    int device;               /* HIP device ordinal */
    uint32_t min_candidates;  /* nodes with fewer candidates are costed on the host; 0 = default */
    uint32_t max_edges;       /* edges per half-mesh on the device; 0 = default (the compiled capacity); may only lower it */
} HprtBuildDeviceOpts;
typedef struct HprtBuildDeviceStats {
    uint64_t nodes_device, candidates_device, candidates_recosted_on_host, nodes_host;   /* nodes_host: costed nodes that took the host path */
    double seconds_device;    /* wall time of the device costing calls, staging and repair included */
} HprtBuildDeviceStats;
/* opts NULL: device 0 and the defaults; stats may be NULL */
int hprt_rbsp_build_device(const HprtModel *m, const HprtRbspParams *params, const HprtBuildDeviceOpts *opts, HprtBuildDeviceStats *stats, HprtRbsp **out);
int hprt_rbsp_build_from_triangles_device(size_t n_tris, const float *p9, const HprtRbspParams *params, const HprtBuildDeviceOpts *opts,
                                          HprtBuildDeviceStats *stats, HprtRbsp **out);
int hprt_rbspkd_build_device(const HprtModel *m, const HprtRbspKdParams *params, const HprtBuildDeviceOpts *opts, HprtBuildDeviceStats *stats,
                             HprtRbspKd **out);
int hprt_rbspkd_build_from_triangles_device(size_t n_tris, const float *p9, const HprtRbspKdParams *params, const HprtBuildDeviceOpts *opts,
                                            HprtBuildDeviceStats *stats, HprtRbspKd **out);

/* ------------------------------------------------------------------------ */
/* Two-level RBSP trees (Accelerator "rbsp" / "rbspkd" on a model with       */
/* object instances).  Stands in for pbrtObjectInstance                      */
/* (core/api.cpp:1794-1819): MakeAccelerator(renderOptions->AcceleratorName, */
/* ...) over the primitives of every object that has more than one (an       */
/* object with exactly one is wrapped as it is, :1798), each wrapped in a    */
/* TransformedPrimitive, and pbrtWorldEnd's top-level accelerator over those */
/* wrappers: an RBSP tree whose leaves hold RBSP trees.  Opt-in:             */
/* hprt_rbsp_build and hprt_rbspkd_build keep refusing such models and the   */
/* front end keeps their BVH and its warning.                                */
/* ------------------------------------------------------------------------ */
typedef struct HprtRbspInst HprtRbspInst;
/* One RBSP tree per object with more than one primitive, over the object's primitives in object space, and the top-level tree
 * over the top-level items in creation order; an instance is bounded by TransformedPrimitive::WorldBound
 * (core/primitive.h:116-118) and projected through the 8 corners of that bound (Primitive::getBounds, core/primitive.h:72-80).
 * Every tree takes the same parameters — params, or with NULL those of the scene's Accelerator line; maxdepth -1 resolves per
 * tree from its own primitive count — so all share M and one direction table.  hprt_rbspkdinst_build builds kd-aware trees
 * (RBSPKd's cost model); the handle remembers which.  HPRT_E_UNSUPPORTED for a model without instances (the job of
 * hprt_rbsp_build / hprt_rbspkd_build), for an M that is not 3, 7, 9 or 13, and when depth(top) + deepest object depth + 1
 * exceeds HPRT_RBSP_MAX_DEPTH: the walk keeps both levels' todo entries and one saved top-level position in one list.  The
 * device-assisted build is not offered for these trees. */
int hprt_rbspinst_build(const HprtModel *m, const HprtRbspParams *params, HprtRbspInst **out);
int hprt_rbspkdinst_build(const HprtModel *m, const HprtRbspKdParams *params, HprtRbspInst **out);
/* info[0..3] = nodes, leaves, primitive references, depth of the top-level tree; info[4] = object definitions, info[5] =
 * object trees (objects with more than one primitive), info[6] = the deepest object tree's depth, info[7] = instances,
 * info[8] = M (directions), info[9] = 1 for kd-aware trees */
int hprt_rbspinst_info(const HprtRbspInst *t, uint32_t info[10]);
/* info[0..3] as above for the tree of object definition `object`; all zero for an object of one primitive, which has no
 * tree (core/api.cpp:1798). */
int hprt_rbspinst_object_info(const HprtRbspInst *t, uint32_t object, uint32_t info[4]);
/* The arrays of the top-level tree / of one object's tree, as hprt_rbsp_copy returns them (any may be NULL); the direction
 * table is every tree's. */
int hprt_rbspinst_copy(const HprtRbspInst *t, void *nodes8, uint32_t *prim_indices, float *directions);
int hprt_rbspinst_object_copy(const HprtRbspInst *t, uint32_t object, void *nodes8, uint32_t *prim_indices);
void hprt_rbspinst_destroy(HprtRbspInst *t);

/* ------------------------------------------------------------------------ */
/* General BSP tree (Accelerator "bsppaper").  Stands in for                */
/* BSPPaper::buildTree (accelerators/bspPaper.cpp:34-305), the BSP tree of  */
/* Ize, Wald and Parker (2008): split planes are the three axis planes and, */
/* per triangle, its own plane and the three planes through its edges       */
/* perpendicular to it; the node's k-DOP (whose direction list grows along  */
/* the path) is the surface of the cost model, and a BVH over the node's    */
/* primitives counts them for a triangle plane.  Byte-identical to the      */
/* reference's 20-byte BSPNode[] (word 0 split / onePrimitive /             */
/* primitiveIndicesOffset; word 1 flags: leaf 1 | nPrims << 1, interior     */
/* aboveChild << 1; words 2-4 the split axis, zero for leaves) and          */
/* primitiveIndices.  "nbDirections" only feeds a statistic and is ignored. */
/* ------------------------------------------------------------------------ */
typedef struct HprtBspPaper HprtBspPaper;
typedef struct HprtBspPaperParams {
    int isect_cost;     /* "intersectcost", default 80 */
    int trav_cost;      /* "traversalcost", default 5 */
    float empty_bonus;  /* "emptybonus", default 0 */
    int max_prims;      /* "maxprims", default 1 */
    int max_depth;      /* "maxdepth", default -1 = round(2 + 1.6 Log2Int(N)) */
    int threads;        /* builder threads (0: OMP_NUM_THREADS, else 16; at most 16); the tree does not depend on it */
} HprtBspPaperParams;
/* params NULL: the scene's Accelerator line (baked models report "bvh" and get the defaults).  Models with object
 * instances: HPRT_E_UNSUPPORTED.  A tree deeper than HPRT_BSPPAPER_MAX_DEPTH: HPRT_E_UNSUPPORTED. */
int hprt_bsppaper_build(const HprtModel *m, const HprtBspPaperParams *params, HprtBspPaper **out);
/* The same over n triangles (9 floats each: three world-space vertices, creation order); params NULL: the defaults. */
int hprt_bsppaper_build_from_triangles(size_t n_tris, const float *p9, const HprtBspPaperParams *params, HprtBspPaper **out);
/* info[0..5] = nodes, leaves, depth (interior levels of the deepest path), primitive references (primitiveIndices entries),
 * interior nodes of the axis sweep, interior nodes on a triangle's plane */
int hprt_bsppaper_info(const HprtBspPaper *t, uint32_t info[6]);
#define HPRT_BSPPAPER_MAX_DEPTH 64     /* the device walk's todo capacity: pbrt's maxTodo (BSP.cpp) */
/* nodes20: info[0] * 20 bytes (5 words per node, the reference's BSPNode); prim_indices: info[3] uint32 (either may be NULL) */
int hprt_bsppaper_copy(const HprtBspPaper *t, void *nodes20, uint32_t *prim_indices);
void hprt_bsppaper_destroy(HprtBspPaper *t);

/* ------------------------------------------------------------------------ */
/* kd-aware general BSP tree (Accelerator "bsppaperkd").  Stands in for     */
/* BSPPaperKd::buildTree (accelerators/bspPaperKd.cpp:34-339) over BSPKd    */
/* and BSPKdNode (accelerators/BSPKd.h:11-193): the bsppaper tree's         */
/* candidates and k-DOP cost model, with axis splits costed                 */
/* kd_trav_cost + C_isect and triangle-plane splits                         */
/* 0.1 * isect_cost * (N - 1) + kd_trav_cost + C_isect; a second minimum,   */
/* trav_cost + C_isect over the plane splits, takes part in the leaf tests  */
/* and supplies the split only where the first minimum is unset.  Nodes are */
/* the reference's 20-byte BSPKdNode[]: word 0 as bsppaper's; word 1 flags, */
/* whose low 3 bits are 0-2 a kd interior node with that axis, 3 a leaf,    */
/* 4 a plane interior node, with aboveChild / nPrims << 3; words 2-4 the    */
/* split axis of a plane node, zero for kd nodes and leaves (the reference  */
/* leaves those uninitialised).  A handle of its own: a bsppaperkd tree is  */
/* walked with the kd form at kd nodes and can never reach the bsppaper     */
/* walk.  "nbDirections" only feeds a statistic and is ignored.             */
/* ------------------------------------------------------------------------ */
typedef struct HprtBspPaperKd HprtBspPaperKd;
typedef struct HprtBspPaperKdParams {
    int isect_cost;     /* "intersectcost", default 80 */
    int trav_cost;      /* "traversalcost", default 5 */
    int kd_trav_cost;   /* "kdtraversalcost", default 1 */
    float empty_bonus;  /* "emptybonus", default 0 */
    int max_prims;      /* "maxprims", default 1 */
    int max_depth;      /* "maxdepth", default -1 = round(2 + 1.6 Log2Int(N)) */
    int threads;        /* builder threads (0: OMP_NUM_THREADS, else 16; at most 16); the tree does not depend on it */
} HprtBspPaperKdParams;
/* As hprt_bsppaper_build (CreateBSPPaperKdTreeAccelerator, accelerators/bspPaperKd.cpp:341-353): params NULL takes the scene's
 * Accelerator line; instanced models and trees deeper than HPRT_BSPPAPERKD_MAX_DEPTH are HPRT_E_UNSUPPORTED. */
int hprt_bsppaperkd_build(const HprtModel *m, const HprtBspPaperKdParams *params, HprtBspPaperKd **out);
int hprt_bsppaperkd_build_from_triangles(size_t n_tris, const float *p9, const HprtBspPaperKdParams *params, HprtBspPaperKd **out);
/* info[0..5] = nodes, leaves, depth, primitive references (hprt_bsppaper_info's slots), kd interior nodes (nbKdNodes), plane
 * interior nodes (nbBSPNodes) */
int hprt_bsppaperkd_info(const HprtBspPaperKd *t, uint32_t info[6]);
#define HPRT_BSPPAPERKD_MAX_DEPTH 64   /* the device walk's todo capacity: pbrt's maxTodo (BSPKd.cpp:36) */
/* nodes20: info[0] * 20 bytes (5 words per node, the reference's BSPKdNode); prim_indices: info[3] uint32 (either may be NULL) */
int hprt_bsppaperkd_copy(const HprtBspPaperKd *t, void *nodes20, uint32_t *prim_indices);
void hprt_bsppaperkd_destroy(HprtBspPaperKd *t);

/* ------------------------------------------------------------------------ */
/* Device-assisted builds of the two general BSP trees (opt-in).  They      */
/* stand in for the same BSPPaper::buildTree / BSPPaperKd::buildTree and    */
/* return the same bytes as hprt_bsppaper_build / hprt_bsppaperkd_build:    */
/* the axis sweep and its sorts, the BVH over a node's primitives, the      */
/* first-minimum scan, the leaf tests, the winner's cut and the             */
/* classification stay on the host; what moves to the GPU is the costing of */
/* a node's split candidates (the extent test of a triangle's plane,        */
/* KDOPMeshWithDirections::cut + KDOPSurfaceArea of                         */
/* accelerators/kDOPMesh.h, BVHAccel::getAmountToLeftAndRight of            */
/* accelerators/bvh.cpp:439-470 and the cost formulas of                    */
/* bspPaper.cpp / bspPaperKd.cpp), one candidate per lane, for nodes with   */
/* at least min_candidates candidates.  A candidate that outgrows one of    */
/* the kernel's fixed capacities is costed again on the host; a node whose  */
/* own mesh or direction list does is costed on the host whole.  Same       */
/* handles: info, copy, attach and the walks are unchanged.  Refusals are   */
/* those of the host entries; without a HIP device: HPRT_E_NO_DEVICE and    */
/* *out stays NULL.  Two-level trees are not offered.                       */
/* ------------------------------------------------------------------------ */
typedef struct HprtBspBuildDeviceOpts {
    int device;               /* HIP device ordinal */
    uint32_t min_candidates;  /* nodes with fewer candidates are costed on the host; 0 = default */
    uint32_t max_edges;       /* edges per half-mesh on the device; 0 = default (the compiled capacity); may only lower it */
    uint32_t max_faces;       /* faces of a child's k-DOP that own an edge, plus the cut's two; 0 = default; may only lower it */
    uint32_t max_face_edges;  /* entries of one face's edge list; 0 = default; may only lower it */
    uint32_t max_stack;       /* entries of the stack that walks the node's BVH; 0 = default; may only lower it */
} HprtBspBuildDeviceOpts;
/* opts NULL: device 0 and the defaults; stats may be NULL */
int hprt_bsppaper_build_device(const HprtModel *m, const HprtBspPaperParams *params, const HprtBspBuildDeviceOpts *opts, HprtBuildDeviceStats *stats,
                               HprtBspPaper **out);
int hprt_bsppaper_build_from_triangles_device(size_t n_tris, const float *p9, const HprtBspPaperParams *params, const HprtBspBuildDeviceOpts *opts,
                                              HprtBuildDeviceStats *stats, HprtBspPaper **out);
int hprt_bsppaperkd_build_device(const HprtModel *m, const HprtBspPaperKdParams *params, const HprtBspBuildDeviceOpts *opts, HprtBuildDeviceStats *stats,
                                 HprtBspPaperKd **out);
int hprt_bsppaperkd_build_from_triangles_device(size_t n_tris, const float *p9, const HprtBspPaperKdParams *params, const HprtBspBuildDeviceOpts *opts,
                                                HprtBuildDeviceStats *stats, HprtBspPaperKd **out);

/* ------------------------------------------------------------------------ */
/* Two-level general BSP trees (Accelerator "bsppaper" / "bsppaperkd" on a  */
/* model with object instances).  Stands in for pbrtObjectInstance          */
/* (core/api.cpp:1794-1819): MakeAccelerator(renderOptions->AcceleratorName,*/
/* ...) over the primitives of every object that has more than one (an      */
/* object with exactly one is wrapped as it is, :1798), each wrapped in a   */
/* TransformedPrimitive, and pbrtWorldEnd's top-level accelerator over      */
/* those wrappers: a general BSP tree whose leaves hold general BSP trees.  */
/* Opt-in: hprt_bsppaper_build and hprt_bsppaperkd_build keep refusing such */
/* models and the front end keeps their BVH and its warning.                */
/* ------------------------------------------------------------------------ */
typedef struct HprtBspPaperInst HprtBspPaperInst;
/* One tree per object with more than one primitive, over the object's primitives in object space (BSPPaper::buildTree,
 * accelerators/bspPaper.cpp:34-305; a triangle offers its object-space planes), and the top-level tree over the top-level items in
 * creation order.  There an instance is a TransformedPrimitive bounded by its WorldBound (core/primitive.h:116-118): it inherits
 * Primitive::getBSPPaperPlanes (core/primitive.h:92-95: no planes) and Primitive::getBounds (core/primitive.h:72-80: the 8 corners
 * of that bound), so it contributes axis candidates only and is classified under a triangle's plane by those corners.  Every tree
 * takes the same parameters — params, or with NULL those of the scene's Accelerator line; maxdepth -1 resolves per tree from its
 * own primitive count.  hprt_bsppaperkdinst_build builds kd-aware trees (BSPPaperKd::buildTree, accelerators/bspPaperKd.cpp:34-339,
 * over BSPKdNode); the handle remembers which.  HPRT_E_UNSUPPORTED for a model without instances (the job of hprt_bsppaper_build /
 * hprt_bsppaperkd_build) and when depth(top) + deepest object depth + 1 exceeds HPRT_BSPPAPER_MAX_DEPTH (=
 * HPRT_BSPPAPERKD_MAX_DEPTH): the walk keeps both levels' todo entries and one saved top-level position in one list. */
int hprt_bsppaperinst_build(const HprtModel *m, const HprtBspPaperParams *params, HprtBspPaperInst **out);
int hprt_bsppaperkdinst_build(const HprtModel *m, const HprtBspPaperKdParams *params, HprtBspPaperInst **out);
/* info[0..7] as hprt_rbspinst_info's: nodes, leaves, primitive references, depth of the top-level tree; object definitions, object
 * trees, the deepest object tree's depth, instances.  info[8] = 1 for kd-aware trees, info[9] = interior nodes of the axis sweep
 * (kd-aware: kd interior nodes, nbKdNodes) over all trees, info[10] = interior nodes on a triangle's plane (nbBSPNodes) over all
 * trees, info[11] = 0 (reserved) */
int hprt_bsppaperinst_info(const HprtBspPaperInst *t, uint32_t info[12]);
/* info[0..3] as above for the tree of object definition `object`; all zero for an object of one primitive, which has no
 * tree (core/api.cpp:1798). */
int hprt_bsppaperinst_object_info(const HprtBspPaperInst *t, uint32_t object, uint32_t info[4]);
/* The arrays of the top-level tree / of one object's tree, as hprt_bsppaper_copy / hprt_bsppaperkd_copy return them: nodes20 is
 * 5 words per node, the reference's BSPNode (BSP.h:122-184) or BSPKdNode (BSPKd.h:11-57); either may be NULL. */
int hprt_bsppaperinst_copy(const HprtBspPaperInst *t, void *nodes20, uint32_t *prim_indices);
int hprt_bsppaperinst_object_copy(const HprtBspPaperInst *t, uint32_t object, void *nodes20, uint32_t *prim_indices);
void hprt_bsppaperinst_destroy(HprtBspPaperInst *t);

/* ------------------------------------------------------------------------ */
/* Node-based BSP trees (Accelerator "bsparbitrary", "bspcluster",          */
/* "bsprandom", and each with "withkd" or "fastkd" appended).  Stand in for */
/* BSPNodeBased::buildTree (accelerators/bspNodeBased.cpp:27-223),          */
/* BSPNodeBasedWithKd::buildTree (bspNodeBasedWithKd.cpp) and               */
/* BSPNodeBasedFastKd::buildTree (bspNodeBasedFastKd.cpp:28-330): at every  */
/* node K split directions are chosen — the PositiveX normals of K drawn    */
/* primitives (chooseArbitraryNormals, randomNormals.h:13-26), the k-means  */
/* of the node's normals (calculateClusterMeans, clustering.h:53-112) or K  */
/* uniform directions (chooseRandomDirections, randomNormals.h:28-46) — and */
/* each is swept like a kd axis over a k-DOP cost model.  The withkd form   */
/* puts the three axes in front of K - 3 chosen directions; the fastkd form */
/* costs the axes kd_trav_cost + C_isect and the chosen directions          */
/* 0.1 * isect_cost * (N - 1) + kd_trav_cost + C_isect, with a second       */
/* minimum trav_cost + C_isect over the chosen directions.  No handles of   */
/* their own: a plain or withkd tree is the reference's BSP over BSPNode,   */
/* structurally a bsppaper tree (HprtBspPaper); a fastkd tree is its BSPKd  */
/* over BSPKdNode, structurally a bsppaperkd tree (HprtBspPaperKd).  Info,  */
/* copy, destroy, attach, counters and pixel maps are those handles'.       */
/* THE ONE DELIBERATE DEPARTURE FROM THE REFERENCE: it seeds std::mt19937    */
/* from std::random_device (bspNodeBased.cpp:28-29), so no two of its       */
/* builds agree; here the engine takes `seed`, default                      */
/* HPRT_BSPNODE_DEFAULT_SEED, so a scene file renders the same tree every   */
/* time.  Everything else is drawn from the engine as the reference draws.  */
/* ------------------------------------------------------------------------ */
#define HPRT_BSPNODE_ARBITRARY 0
#define HPRT_BSPNODE_CLUSTER 1
#define HPRT_BSPNODE_RANDOM 2
#define HPRT_BSPNODE_PLAIN 0
#define HPRT_BSPNODE_WITHKD 1
#define HPRT_BSPNODE_FASTKD 2
#define HPRT_BSPNODE_DEFAULT_SEED 5489u   /* std::mt19937::default_seed */
typedef struct HprtBspNodeParams {
    int chooser;        /* HPRT_BSPNODE_ARBITRARY / _CLUSTER / _RANDOM: the accelerator's name */
    int form;           /* HPRT_BSPNODE_PLAIN / _WITHKD / _FASTKD: the name's suffix */
    int n_directions;   /* "nbDirections" (K), default 3; withkd and fastkd need K >= 3 */
    uint32_t seed;      /* "seed", default HPRT_BSPNODE_DEFAULT_SEED */
    int isect_cost;     /* "intersectcost", default 80 */
    int trav_cost;      /* "traversalcost", default 5 */
    int kd_trav_cost;   /* "kdtraversalcost", default 1 (fastkd only) */
    float empty_bonus;  /* "emptybonus", default 0 */
    int max_prims;      /* "maxprims", default 1 */
    int max_depth;      /* "maxdepth", default -1 = round(2 + 1.6 Log2Int(N)) */
    int threads;        /* builder threads (0: OMP_NUM_THREADS, else 16; at most 16); the tree does not depend on it */
} HprtBspNodeParams;
/* Create{BSPArbitrary,BSPCluster,BSPRandom}[WithKd]TreeAccelerator (accelerators/bspCluster.cpp:36-48 and siblings): the plain and
 * withkd forms.  params NULL takes chooser, form and parameters from the scene's Accelerator line.  HPRT_E_UNSUPPORTED where the
 * reference's build is undefined — K < 3 for withkd (its K - 3 wraps), a drawn primitive index equal to the node's primitive
 * count — and for instanced models and trees deeper than HPRT_BSPPAPER_MAX_DEPTH. */
int hprt_bspnode_build(const HprtModel *m, const HprtBspNodeParams *params, HprtBspPaper **out);
int hprt_bspnode_build_from_triangles(size_t n_tris, const float *p9, const HprtBspNodeParams *params, HprtBspPaper **out);
/* Create{BSPArbitrary,BSPCluster,BSPRandom}FastKdTreeAccelerator (accelerators/bspClusterFastKd.cpp:37-50 and siblings): the fastkd
 * form.  As above; also HPRT_E_UNSUPPORTED where only the second minimum is set (the reference then reads edges[-1]) and for trees
 * deeper than HPRT_BSPPAPERKD_MAX_DEPTH. */
int hprt_bspnodekd_build(const HprtModel *m, const HprtBspNodeParams *params, HprtBspPaperKd **out);
int hprt_bspnodekd_build_from_triangles(size_t n_tris, const float *p9, const HprtBspNodeParams *params, HprtBspPaperKd **out);
/* Device-assisted builds of the node-based trees (opt-in).  They return the same bytes, the same refusals and the same messages as
 * the four entries above: the direction chooser (k-means included) and its draws, the projections, sorts and sweeps, the
 * first-minimum scans, the leaf tests, the winner's cut and the classification stay on the host; what moves to the GPU is the
 * costing of a node's split candidates (KDOPMeshWithDirections::cut + KDOPSurfaceArea of accelerators/kDOPMesh.h and the cost
 * formulas of bspNodeBased.cpp / bspNodeBasedFastKd.cpp), one candidate per lane, for nodes with at least min_candidates
 * candidates.  A candidate that outgrows one of the kernel's fixed capacities is costed again on the host; a node whose own mesh or
 * direction list does, or which sweeps more than 16 directions, is costed on the host whole.  opts NULL: device 0 and the defaults;
 * max_stack is not read (these trees have no node BVH); stats may be NULL.  Without a HIP device: HPRT_E_NO_DEVICE and *out stays
 * NULL; what the host entry refuses before it looks at a primitive (bad arguments, an instanced model, the wrong form, a K the
 * reference's build is undefined for) is refused first, with the same code and message, on every machine. */
int hprt_bspnode_build_device(const HprtModel *m, const HprtBspNodeParams *params, const HprtBspBuildDeviceOpts *opts, HprtBuildDeviceStats *stats,
                              HprtBspPaper **out);
int hprt_bspnode_build_from_triangles_device(size_t n_tris, const float *p9, const HprtBspNodeParams *params, const HprtBspBuildDeviceOpts *opts,
                                             HprtBuildDeviceStats *stats, HprtBspPaper **out);
int hprt_bspnodekd_build_device(const HprtModel *m, const HprtBspNodeParams *params, const HprtBspBuildDeviceOpts *opts, HprtBuildDeviceStats *stats,
                                HprtBspPaperKd **out);
int hprt_bspnodekd_build_from_triangles_device(size_t n_tris, const float *p9, const HprtBspNodeParams *params, const HprtBspBuildDeviceOpts *opts,
                                               HprtBuildDeviceStats *stats, HprtBspPaperKd **out);

/* ------------------------------------------------------------------------ */
/* Two-level node-based BSP trees (the nine names above on a model with     */
/* object instances).  Stands in for pbrtObjectInstance                     */
/* (core/api.cpp:1794-1819) and pbrtWorldEnd under those accelerators, as   */
/* the two-level general BSP trees do: a node-based tree whose leaves hold  */
/* node-based trees.  Opt-in: hprt_bspnode_build and hprt_bspnodekd_build   */
/* keep refusing such models, the front end keeps their BVH and its warning.*/
/* ------------------------------------------------------------------------ */
/* One entry for all nine names: the handle is an HprtBspPaperInst — kd-aware (BSPKdNode words) for HPRT_BSPNODE_FASTKD, plain
 * (BSPNode words; a withkd tree's axis splits are plane nodes with a unit axis) for the other two forms — and hprt_bsppaperinst_info /
 * _object_info / _copy / _object_copy / _destroy and hprt_scene_attach_bsppaperinst serve it as they are.  params NULL takes
 * chooser, form and parameters from the scene's Accelerator line (HPRT_E_INVALID when it names no node-based tree).  One tree per
 * object with more than one primitive, over the object's primitives in object space, and the top-level tree over the top-level
 * items in creation order; every tree takes the same parameters, maxdepth -1 resolving per tree.  What the reference's builds call
 * on a primitive is WorldBound, getBounds(direction) and, through the direction choosers, Normal; getSurfaceArea is not among them
 * (only the debugging dump of genericBSP.h:107-130 calls it).  On the top level an instance is a TransformedPrimitive
 * (core/primitive.h:144-182): its Normal() is (0, 0, 0) (:170-172), its getBounds is Primitive's over the 8 corners of its
 * WorldBound (:72-82, :166-168), its getSurfaceArea() forwards to the wrapped primitive (:174-176) and is never asked.  So an
 * instance offers the choosers a zero normal — chooseArbitraryNormals then returns zero vectors, which have no candidate;
 * calculateClusterMeans clusters them at Angle = acos(0) and normalises zero sums — and the library does what the reference's code
 * does with those values, refusing only where that code indexes past an array (as hprt_bspnode_build does).
 * THE SEED RULE: every tree of the handle starts a fresh std::mt19937(seed).  This is the one deliberate departure from the
 * reference stated above (it seeds each tree's engine from std::random_device), applied per tree, and no second one.
 * Refusals, in this order: a null argument (HPRT_E_INVALID); a model without instances (HPRT_E_UNSUPPORTED: the job of
 * hprt_bspnode_build / hprt_bspnodekd_build); parameters the reference's build is undefined for, before any primitive is looked at;
 * a tree's own refusal, prefixed "object N:" or "top level:"; depth(top) + deepest object depth + 1 above HPRT_BSPPAPER_MAX_DEPTH
 * (= HPRT_BSPPAPERKD_MAX_DEPTH). */
int hprt_bspnodeinst_build(const HprtModel *m, const HprtBspNodeParams *params, HprtBspPaperInst **out);
/* The device-assisted build of the same handle: the same bytes, refusals and messages.  The costing hook is installed once and ONE
 * device session serves every tree; k_sweepcost costs the candidates of nodes with at least min_candidates candidates, overflowing
 * candidates are costed again on the host, and stats (may be NULL) are summed over the trees.  Without a HIP device:
 * HPRT_E_NO_DEVICE after the refusals that do not depend on a device or a primitive (the first three above), *out stays NULL. */
int hprt_bspnodeinst_build_device(const HprtModel *m, const HprtBspNodeParams *params, const HprtBspBuildDeviceOpts *opts, HprtBuildDeviceStats *stats,
                                  HprtBspPaperInst **out);

/* ------------------------------------------------------------------------ */
/* Device scene.  Upload step that follows the BVH build: stands in for the  */
/* `primitives`/`nodes` members BVHAccel keeps (accelerators/bvh.h:69-79) and */
/* the Scene object (core/scene.h:50-80).  The library copies everything to   */
/* HBM and owns that memory until hprt_scene_destroy.                         */
/* ------------------------------------------------------------------------ */
typedef struct HprtScene HprtScene;

typedef struct HprtShapeDesc {       /* one Shape directive (core/api.cpp:1561-1651) */
    int32_t kind;                    /* 0 triangle mesh, 1 sphere */
    int32_t material;                /* index into materials */
    int32_t area_light;              /* index into lights or -1 (GeometricPrimitive::areaLight).  A mesh is n_tris Triangle shapes, each with
                                      * a DiffuseAreaLight of its own (core/api.cpp:1609-1636): lights area_light .. area_light + n_tris - 1,
                                      * in face order, each with .shape = this shape */
    int32_t reverse_orientation, transform_swaps_handedness; /* core/shape.h:79-80 */
    /* mesh: world-space arrays as TriangleMesh holds them (shapes/triangle.cpp:54-92) */
    uint32_t n_tris, n_verts;
    const int32_t *indices;          /* 3*n_tris */
    const float *P;                  /* 3*n_verts */
    const float *N;                  /* 3*n_verts or NULL */
    const float *UV;                 /* 2*n_verts or NULL */
    const float *S;                  /* 3*n_verts or NULL */
    /* sphere (shapes/sphere.h:50-59) */
    float object_to_world[16], world_to_object[16];
    float radius, z_min, z_max, theta_min, theta_max, phi_max;
} HprtShapeDesc;

typedef struct HprtMaterialDesc {    /* materials/matte.cpp:64-72, materials/plastic.cpp:72-84, materials/mirror.cpp:58-64 */
    int32_t type;                    /* 0 matte (sigma != 0: OrenNayar), 1 plastic, 2 mirror (Kr in Ks), 3 substrate (roughness = uroughness,
                                      * sigma = vroughness; materials/substrate.cpp), 4 metal (Kd = eta, Ks = k, roughness / sigma likewise;
                                      * materials/metal.cpp), 5 glass (Kd = Kt, Ks = Kr, roughness = eta; sigma = uroughness and Kr[0] = vroughness — both 0: the smooth FresnelSpecular
                                      * lobe, else MicrofacetReflection + MicrofacetTransmission; materials/glass.cpp:61-93), 6 uber (below) */
    float Kd[3], sigma, Ks[3], roughness;
    int32_t remap_roughness;
    int32_t kd_texture, ks_texture;  /* index into HprtSceneDesc::textures when Kd / Ks is an image texture, else -1 */
    /* type 6, UberMaterial (materials/uber.cpp): Kd, Ks as named, roughness = uroughness, sigma = vroughness, and the lobes only it
     * has: Kr (specular reflection), Kt (specular transmission), opacity (1 - opacity passes straight through), eta */
    float Kr[3], Kt[3], opacity[3], eta;
    int32_t opacity_texture;         /* uber: "opacity" as an image texture (materials/uber.cpp:53, scenes/livingroom:30), else -1 */
} HprtMaterialDesc;

/* ImageTexture<RGBSpectrum, Spectrum> (textures/imagemap.h:71-122) with its built MIPMap (core/mipmap.h):
 * level 0 is the power-of-two image after ImageTexture::GetTexture's conversion (scale, inverse gamma, y flip:
 * (0,0) is the lower left texel), level k the 2x2 box filter of level k-1; rgb holds 3*w*h floats per level. */
typedef struct HprtTextureLevel { int32_t w, h; const float *rgb; } HprtTextureLevel;
typedef struct HprtTextureDesc {
    const HprtTextureLevel *levels; uint32_t n_levels;
    int32_t trilinear;               /* "trilinear" (default false: EWA, core/mipmap.h:262-290) */
    float max_anisotropy;            /* "maxanisotropy", 8 */
    int32_t wrap;                    /* 0 repeat, 1 black, 2 clamp */
    float su, sv, du, dv;            /* UVMapping2D (core/texture.cpp:93-99) */
    const float *weight_lut;         /* MIPMap::weightLut, 128 floats */
} HprtTextureDesc;

typedef struct HprtLightDesc {       /* lights/point.cpp, lights/distant.cpp, lights/diffuse.cpp, lights/infinite.cpp */
    int32_t type;                    /* 0 point, 1 distant, 2 diffuse area, 3 infinite */
    float pos[3];                    /* point: pLight (world); distant: wLight (world, normalised) */
    float I[3];                      /* I / L / Lemit */
    int32_t shape;                   /* area light: shape index */
    int32_t two_sided;
    /* infinite: the radiance map is textures[texture] — its texels as InfiniteAreaLight holds them (ReadImage order, not flipped,
     * already multiplied by L * scale; 1x1 for a constant light) — and the light <-> world transform, row-major */
    int32_t texture;
    float light_to_world[16], world_to_light[16];
} HprtLightDesc;

/* Object instancing (pbrtObjectBegin/End/Instance, core/api.cpp:1752-1820; TransformedPrimitive,
 * core/primitive.cpp:70-102).  An object definition owns a contiguous range of `shapes` and the
 * aggregate ObjectInstance builds over their primitives (core/api.cpp:1798-1806; with a single
 * primitive the reference wraps that primitive directly and the one-leaf tree is only used for
 * its bounds).  An instance is one primitive of the top-level aggregate. */
typedef struct HprtObjectDesc {
    uint32_t first_shape, n_shapes;
    const void *nodes; uint32_t n_nodes;            /* LinearBVHNode layout, primitives numbered within the object */
    const uint32_t *prim_order; uint32_t n_prims;
} HprtObjectDesc;
typedef struct HprtInstanceDesc {
    int32_t object;
    float instance_to_world[16], world_to_instance[16];   /* row-major Transform::m / mInv at ObjectInstance */
} HprtInstanceDesc;
typedef struct HprtTopItem {         /* renderOptions->primitives in creation order */
    int32_t kind;                    /* 0: all primitives of shapes[index]; 1: instances[index] */
    uint32_t index;
} HprtTopItem;

typedef struct HprtSceneDesc {
    const void *nodes;               /* n_nodes * 32 B, LinearBVHNode layout: the top-level aggregate */
    uint32_t n_nodes;
    const uint32_t *prim_order;      /* n_prims: ordered position -> creation-order primitive number */
    uint32_t n_prims;
    const HprtShapeDesc *shapes; uint32_t n_shapes;   /* creation order */
    const HprtMaterialDesc *materials; uint32_t n_materials;
    const HprtLightDesc *lights; uint32_t n_lights;
    int32_t light_strategy;
    const HprtTextureDesc *textures; uint32_t n_textures;
    /* instancing; all NULL / 0 without it.  top == NULL: every shape, in order, is top-level */
    const HprtObjectDesc *objects; uint32_t n_objects;
    const HprtInstanceDesc *instances; uint32_t n_instances;
    const HprtTopItem *top; uint32_t n_top;
} HprtSceneDesc;

/* device < 0 selects the current HIP device. */
int hprt_scene_create(const HprtSceneDesc *desc, int device, HprtScene **out);
/* Convenience: the same from a parsed model and its BVH. */
int hprt_scene_create_from_model(const HprtModel *m, const HprtBvh *b, int device, HprtScene **out);
void hprt_scene_destroy(HprtScene *s);
/* Makes the scene walk a kd-tree (KdTreeAccel::Intersect / IntersectP, accelerators/kdtreeaccel.cpp:381-521) from now
 * on: hprt_intersect*, hprt_occluded*, their _device forms and hprt_render.  The tree must be built over this scene's
 * primitives (creation order, the numbering of the BVH's prim_order); it is validated (child offsets, leaf index ranges,
 * primitive count, depth <= HPRT_KD_MAX_DEPTH: else HPRT_E_INVALID / HPRT_E_UNSUPPORTED) and copied to HBM.  Hits keep
 * reporting ORDERED primitive indices (the BVH's numbering) so that shading is unchanged.  Scenes with object instances:
 * HPRT_E_UNSUPPORTED (no two-level kd walk).  Attaching again replaces the tree.
 * Counters of a kd scene: [0] nbNodeTraversals (every node the walk loop visits), [1] kdTreeNodeTraversals (interior
 * nodes), [2] triangle tests, [3] sphere tests; HprtRenderStats::nodes_fetched[_p] / nodes_entered[_p] carry [0] / [1],
 * and HPRT_RENDER_PIXEL_STATS slots 5 / 6 hold kdTreeNodeTraversals[P] (write them with hprt_write_pixel_stats_accel). */
int hprt_scene_attach_kdtree(HprtScene *s, const HprtKdTree *t);
/* The same for an RBSP tree (RBSP::Intersect / IntersectP, accelerators/rbsp.cpp:405-547).  Attaching either tree
 * replaces whichever tree was attached before.  Counters of an RBSP scene: [0] nbNodeTraversals, [1]
 * bspTreeNodeTraversals (interior nodes), [2] triangle tests, [3] sphere tests; HPRT_RENDER_PIXEL_STATS slots 5 / 6 hold
 * bspTreeNodeTraversals[P] (hprt_write_pixel_stats_accel with HPRT_ACCEL_RBSP). */
int hprt_scene_attach_rbsp(HprtScene *s, const HprtRbsp *t);
/* The same for a kd-aware RBSP tree (RBSPKd::Intersect / IntersectP, accelerators/rbspKd.cpp:490-638).  Attaching any of the
 * kd-tree, the RBSP tree and the rbspkd tree replaces whichever was attached before.  Counters of an rbspkd scene: [0]
 * nbNodeTraversals, [1] every interior node (kdTreeNodeTraversals + bspTreeNodeTraversals), [2] triangle tests, [3] sphere
 * tests; HPRT_RENDER_PIXEL_STATS slots 5 / 6 hold every interior node too.  The kd share comes from
 * hprt_scene_kd_counters and hprt_pixel_kd_stats_read. */
int hprt_scene_attach_rbspkd(HprtScene *s, const HprtRbspKd *t);
/* The same for a general BSP tree (BSP::Intersect / IntersectP, accelerators/BSP.cpp:27-165).  Attaching any tree replaces
 * whichever was attached before.  Counters of a bsppaper scene: [0] nbNodeTraversals, [1] bspTreeNodeTraversals (interior
 * nodes), [2] triangle tests, [3] sphere tests; HPRT_RENDER_PIXEL_STATS slots 5 / 6 hold bspTreeNodeTraversals[P]
 * (hprt_write_pixel_stats_accel with HPRT_ACCEL_BSP). */
int hprt_scene_attach_bsppaper(HprtScene *s, const HprtBspPaper *t);
/* The same for a kd-aware general BSP tree (BSPKd::Intersect / IntersectP, accelerators/BSPKd.cpp:25-171).  Attaching any of the
 * five trees replaces whichever was attached before; a refused attach leaves the previous walk in place.  Counters of a
 * bsppaperkd scene follow the rbspkd scene's: [1] and HPRT_RENDER_PIXEL_STATS slots 5 / 6 hold every interior node
 * (kdTreeNodeTraversals + bspTreeNodeTraversals), and the kd share comes from hprt_scene_kd_counters and
 * hprt_pixel_kd_stats_read. */
int hprt_scene_attach_bsppaperkd(HprtScene *s, const HprtBspPaperKd *t);
/* Makes a scene WITH object instances walk two-level kd-trees: KdTreeAccel::Intersect / IntersectP on both levels, joined by
 * TransformedPrimitive::Intersect / IntersectP (core/primitive.cpp:77-102).  The handle must be built from the model the
 * scene was made of: its object and instance counts and every tree's primitive count are checked against the scene's
 * (HPRT_E_INVALID), every tree passes the kd-tree's structural check, and depth(top) + deepest object depth + 1 must not
 * exceed HPRT_KD_MAX_DEPTH (HPRT_E_UNSUPPORTED).  Hit records are the BVH walk's of an instanced scene (ordered primitive
 * over all aggregates, instance index).  Counters follow the kd scene's contract, summed over both levels as r.stats +=
 * ray.stats (core/primitive.cpp:84,100) sums them; an instance entry is not itself a primitive test.  Attaching replaces
 * whichever tree was attached before; an attach refused by these checks leaves the previous walk in place (a device failure
 * during the upload that follows them leaves the scene on its BVH). */
int hprt_scene_attach_kdinst(HprtScene *s, const HprtKdInst *t);
/* The same for two-level RBSP trees: RBSP::Intersect / IntersectP — for a handle of hprt_rbspkdinst_build RBSPKd::Intersect /
 * IntersectP — on both levels, joined by TransformedPrimitive.  The checks are hprt_scene_attach_kdinst's with the RBSP tree's
 * structural check and HPRT_RBSP_MAX_DEPTH; a scene without instances is HPRT_E_UNSUPPORTED.  Counters follow the rbsp scene's
 * contract ([0] every node either walk visits, [1] the interior ones), summed over both levels; for kd-aware trees the kd
 * share (interior nodes of direction < 3, both levels) comes from hprt_scene_kd_counters and hprt_pixel_kd_stats_read exactly
 * as for an rbspkd scene, for plain trees those report zeros. */
int hprt_scene_attach_rbspinst(HprtScene *s, const HprtRbspInst *t);
/* The same for two-level general BSP trees: BSP::Intersect / IntersectP (accelerators/BSP.cpp:27-165) — for a handle of
 * hprt_bsppaperkdinst_build BSPKd::Intersect / IntersectP (accelerators/BSPKd.cpp:25-171) — on both levels, joined by
 * TransformedPrimitive (core/primitive.cpp:77-102); an object's split axes are object-space vectors and meet the instance's
 * transformed ray.  The checks are hprt_scene_attach_kdinst's with CheckBspPaperTree / CheckBspPaperKdTree and
 * HPRT_BSPPAPER_MAX_DEPTH; a scene without instances is HPRT_E_UNSUPPORTED.  Counters follow the bsppaper scene's contract, summed
 * over both levels; for kd-aware trees the kd share (kd interior nodes, both levels) comes from hprt_scene_kd_counters and
 * hprt_pixel_kd_stats_read exactly as for a bsppaperkd scene, for plain trees those report zeros. */
int hprt_scene_attach_bsppaperinst(HprtScene *s, const HprtBspPaperInst *t);
/* kdTreeNodeTraversals (out[0]) and kdTreeNodeTraversalsP (out[1]) of the last counting trace (hprt_intersect / hprt_occluded
 * with counters) or counting render of an rbspkd or bsppaperkd scene, or of a scene with kd-aware two-level RBSP or general BSP trees; zeros
 * for any other scene. */
int hprt_scene_kd_counters(HprtScene *s, uint64_t out[2]);

/* ------------------------------------------------------------------------ */
/* Batched Aggregate interface.  Stand in for                                */
/*   bool BVHAccel::Intersect(const Ray&, SurfaceInteraction*) const         */
/*        (accelerators/bvh.cpp:354-396, core/primitive.h:57-61)             */
/*   bool BVHAccel::IntersectP(const Ray&) const (accelerators/bvh.cpp:398-437) */
/* over n rays held in host memory (SoA-of-arrays: o and d are 3*n floats,   */
/* xyz interleaved per ray).  Closest hit writes the shrunken tMax (unchanged */
/* on a miss), the ORDERED primitive index (-1 on a miss) and b0,b1,b2        */
/* (triangles; 0 for spheres).  counters (may be NULL) receives               */
/* [0] BVH nodes fetched (traversal-loop iterations), [1] nodes entered (the   */
/* reference's "BVH node traversals" counter), [2] triangle tests, [3] sphere  */
/* tests — the figures SURVEY.md §8(d)'s byte model is built from.            */
/* These calls are BATCH interfaces: n = 1 meets the single-ray contract of    */
/* Aggregate::Intersect(const Ray&, SurfaceInteraction*) but costs a host-to-  */
/* device copy, a kernel launch and a copy back (~tens of microseconds) per    */
/* ray — a contract shim for tests, not a usable rendering path.  A host that  */
/* wants images calls hprt_render; one that wants rays answered hands over     */
/* thousands to millions at a time.                                            */
/* ------------------------------------------------------------------------ */
int hprt_intersect(HprtScene *s, size_t n, const float *o, const float *d, const float *tmax, float *t_out,
                   int32_t *prim_out, float *bary_out, uint64_t counters[4]);
int hprt_occluded(HprtScene *s, size_t n, const float *o, const float *d, const float *tmax, uint8_t *occluded_out,
                  uint64_t counters[4]);
/* With object instances (TransformedPrimitive::Intersect, core/primitive.cpp:77-93) the ordered
 * primitive index numbers the primitives of all aggregates — top level first, then object 0, 1, ... —
 * and inst_out (may be NULL) receives the instance the hit went through (index into
 * HprtSceneDesc::instances), -1 for none.  hprt_intersect is this call without inst_out. */
int hprt_intersect_instanced(HprtScene *s, size_t n, const float *o, const float *d, const float *tmax, float *t_out,
                             int32_t *prim_out, int32_t *inst_out, float *bary_out, uint64_t counters[4]);
/* Same with rays/hits already resident in HBM (device pointers, SoA planes:
 * ox,oy,oz,dx,dy,dz,tmax each n floats).  `stream` is a hipStream_t or NULL.
 * Timed by bench.py's kernel microbenchmarks. */
int hprt_intersect_device(HprtScene *s, size_t n, const float *d_rays7, float *d_t, int32_t *d_prim, float *d_bary3,
                          void *stream);
int hprt_occluded_device(HprtScene *s, size_t n, const float *d_rays7, uint8_t *d_occ, void *stream);

/* ------------------------------------------------------------------------ */
/* Integrator.  Stands in for SamplerIntegrator::Render(const Scene&)        */
/* (core/integrator.cpp:230-360) with PathIntegrator::Li                     */
/* (integrators/path.cpp:64-204) as the radiance estimator, the Halton        */
/* sampler (samplers/halton.cpp) and the box-filtered Film                    */
/* (core/film.h:130-170, core/film.cpp:118-132).                              */
/* ------------------------------------------------------------------------ */
typedef struct HprtRenderDesc {
    HprtRenderOptions opt;
    /* 16x16 image tiles [tile_begin, tile_end) of the row-major tile grid
     * (core/integrator.cpp:237-244) are rendered; tile_stride > 1 takes every
     * tile_stride-th tile starting at tile_begin (round-robin sharding across
     * GPUs).  tile_end <= 0 means "all tiles". */
    int32_t tile_begin, tile_end, tile_stride;
    int32_t spp_chunk;             /* samples per pixel per wavefront batch; <= 0: automatic */
    int32_t flags;                 /* HPRT_RENDER_* */
} HprtRenderDesc;
#define HPRT_RENDER_COUNT_WORK 1   /* collect node/triangle counters (slower) */
#define HPRT_RENDER_PIXEL_STATS 2  /* also keep them per pixel: the fork's GeneralStats heat-map data (implies COUNT_WORK) */
/* EstimateDirect's BSDF-sampled ray (core/integrator.cpp:176-190) is only traced to learn whether its closest hit is the
 * emitter.  A plain render does not trace it when a cheap exact test proves that it cannot reach the emitter's sphere
 * (it would add exactly zero), nor the segment that leaves a path's last vertex (the reference intersects it and stops,
 * integrators/path.cpp:97-110): same film, fewer rays.  A counting render traces every ray the reference traces, so that
 * its counters are the reference's — unless COUNT_TRACED asks it to count what a plain render traces.  TRACE_ALL makes a
 * plain render trace the reference's full ray set too. */
#define HPRT_RENDER_COUNT_TRACED 4
#define HPRT_RENDER_TRACE_ALL 8
/* Tile-sharded renders whose films hprt_film_gather will merge: box-filter contributions that cross a tile border
 * (FilmTile pixels outside the tile's own 16x16 block, core/film.cpp:98-103) are not merged into the film but kept as
 * HprtFilmRecords, so that the gather can merge the records of ALL ranks into each pixel in source-tile order. */
#define HPRT_RENDER_EXPORT_FOREIGN 16

typedef struct HprtRenderStats {
    uint64_t camera_rays;          /* nCameraRays, core/integrator.cpp:48,293 */
    uint64_t rays;                 /* "Regular ray intersection tests", core/scene.cpp:40,47 */
    uint64_t shadow_rays;          /* "Shadow ray intersection tests",  core/scene.cpp:42,53 */
    uint64_t nodes_fetched, nodes_fetched_p;   /* traversal-loop iterations (closest / any hit) */
    uint64_t nodes_entered, nodes_entered_p;   /* nbNodeTraversals / nbNodeTraversalsP, bvh.cpp:48-49 */
    uint64_t tri_tests, tri_tests_p;           /* nTests / nTestsP, shapes/triangle.cpp:43-44 */
    uint64_t sphere_tests, sphere_tests_p;
    double render_seconds;         /* the reference's Timings/Rendertime span: tile loop only */
    double extend_seconds, occluded_seconds;  /* HIP-event time inside the traversal kernels */
    uint64_t extend_launches, occluded_launches;
    uint64_t extend_rays, occluded_rays;
} HprtRenderStats;

/* Renders into the scene's film.  d_film_xyzw, if not NULL, is a caller-owned
 * DEVICE buffer of 4*W*H floats (W,H = cropped pixel bounds) that receives the
 * merged film state (xyz, filterWeightSum) of the rendered tiles and zeros
 * elsewhere — what Film::MergeFilmTile leaves in Film::pixels.  Summing such
 * buffers over GPUs (RCCL reduce) reproduces the single-GPU film exactly. */
int hprt_render(HprtScene *s, const HprtRenderDesc *desc, float *d_film_xyzw, void *stream, HprtRenderStats *stats);
/* Optional: allocate everything the coming hprt_render(s, desc, ...) needs in HBM now (the wavefront workspace is
 * ~365 B per path of a batch: 98 GB for the 256 M-path batches of a 700x700, 1,024 spp frame), so that a host that
 * renders once (pbrt does: Integrator::Render, core/api.cpp:1851) pays the allocation at scene load — next to
 * BVHAccel's own node allocation (accelerators/bvh.cpp:181) — not inside Render().  A later render with a
 * description that needs more simply grows the buffers. */
int hprt_scene_reserve(HprtScene *s, const HprtRenderDesc *desc);
/* Pixel::stats (core/film.h:91; GeneralStats, core/geometry.h:1078-1173) of the last hprt_render that had
 * HPRT_RENDER_PIXEL_STATS set: per film pixel, row-major over the cropped pixel bounds, 7 values —
 * rays (= samples), primitiveIntersections, primitiveIntersectionsP, leafNodeTraversals,
 * leafNodeTraversalsP, bvhTreeNodeTraversals, bvhTreeNodeTraversalsP — every ray of a pixel's samples
 * adds its counters once (core/integrator.cpp:327-328, integrators/path.cpp:92-200, core/light.cpp:62).
 * Pixels of tiles that were not rendered hold zeros, so per-rank results add up like the film. */
int hprt_pixel_stats_read(HprtScene *s, uint64_t *out7, size_t n_pixels);
/* For a render of an rbspkd or bsppaperkd scene with HPRT_RENDER_PIXEL_STATS: the per-pixel kd share of slots 5 / 6, as two planes
 * (out2[0 .. n) kdTreeNodeTraversals, out2[n .. 2n) kdTreeNodeTraversalsP), row-major like hprt_pixel_stats_read. */
int hprt_pixel_kd_stats_read(HprtScene *s, uint64_t *out2, size_t n_pixels);
/* Film::WriteGeneralStats (core/film.cpp:170-264): writes <prefix>-primitiveIntersections.txt,
 * -primitiveIntersectionsP.txt, -leafNodeTraversals.txt, -leafNodeTraversalsP.txt (one row of the
 * image per line, values separated by blanks) and the all-zero kd-tree / BSP matrices the fork
 * writes for a BVH render.  Its -renderTime.txt (wall-clock per pixel) has no counterpart here. */
int hprt_write_pixel_stats(const char *prefix, const uint64_t *stats7, int width, int height);
/* The same for a render of either accelerator: accel 0 (BVH) writes what hprt_write_pixel_stats writes; accel 1 (kd-tree)
 * writes slots 5 / 6 to -kdTreeNodeTraversals.txt / -kdTreeNodeTraversalsP.txt, as the fork does for a kd render (the
 * BSP matrices stay zero). */
#define HPRT_ACCEL_BVH 0
#define HPRT_ACCEL_KDTREE 1
#define HPRT_ACCEL_RBSP 2          /* slots 5 / 6 go to -bspTreeNodeTraversals[P].txt (core/film.cpp:176-177) */
#define HPRT_ACCEL_BSP HPRT_ACCEL_RBSP     /* the general BSP tree (bsppaper): its interior nodes are bspTreeNodeTraversals too */
int hprt_write_pixel_stats_accel(const char *prefix, const uint64_t *stats7, int width, int height, int accel);
/* The same for an rbspkd or bsppaperkd render: -kdTreeNodeTraversals[P].txt from kd2 (hprt_pixel_kd_stats_read's two planes) and
 * -bspTreeNodeTraversals[P].txt = slot 5 / 6 minus the kd share, as Film::WriteGeneralStats does (core/film.cpp:174-177). */
int hprt_write_pixel_stats_rbspkd(const char *prefix, const uint64_t *stats7, const uint64_t *kd2, int width, int height);
/* Film::WriteImage arithmetic (core/film.cpp:266-303) on a host copy of a film
 * state: rgb_out = 3*W*H floats, top row first. */
int hprt_film_resolve(const float *xyzw, size_t n_pixels, float film_scale, float *rgb_out);
/* Film state of the last hprt_render on this scene, copied to the host. */
int hprt_film_read(HprtScene *s, float *xyzw_out, size_t n_pixels);
/* imageio.cpp:437+ : PFM writer (bottom row first, little endian). */
int hprt_write_pfm(const char *path, const float *rgb, int width, int height);

/* ------------------------------------------------------------------------ */
/* Multi-GPU film gather.  Stands in for Film::MergeFilmTile                  */
/* (core/film.cpp:118-132) across GPUs: the reference merges every worker's   */
/* FilmTile into Film::pixels under a mutex; here rank r of n renders tiles   */
/* r, r+n, ... (HprtRenderDesc::tile_begin / tile_stride) with                */
/* HPRT_RENDER_EXPORT_FOREIGN and ONE RCCL step over xGMI lands the frame on  */
/* the root: ncclReduce(sum) of the per-rank films (disjoint addends: exact)  */
/* then a grouped ncclSend/ncclRecv of the few cross-tile records, which the  */
/* root adds per pixel in ascending source-tile order — the order of the      */
/* single-GPU film, so the n-GPU film equals it bit for bit.                  */
/* ------------------------------------------------------------------------ */
typedef struct HprtComm HprtComm;
#define HPRT_COMM_ID_BYTES 128
/* One process per GPU: rank 0 draws an id (ncclGetUniqueId), the host program hands the 128 bytes to every
 * rank by whatever means it has, and every rank creates its communicator (ncclCommInitRank) on `device`
 * (< 0: the current HIP device).  RCCL refuses two ranks on one device. */
int hprt_comm_unique_id(uint8_t id[HPRT_COMM_ID_BYTES]);
int hprt_comm_create(const uint8_t id[HPRT_COMM_ID_BYTES], int rank, int n_ranks, int device, HprtComm **out);
/* rank, size and device as the communicator reports them (ncclCommUserRank / Count / CuDevice); any may be NULL */
int hprt_comm_info(const HprtComm *c, int *rank, int *n_ranks, int *device);
void hprt_comm_destroy(HprtComm *c);
/* Collective over the communicator, after each rank's hprt_render(..., HPRT_RENDER_EXPORT_FOREIGN).  d_film_xyzw is the
 * DEVICE buffer that render wrote (NULL: whichever buffer it wrote — the caller's or the scene's own; a different
 * pointer is refused); on return the root's buffer holds the merged frame (what Film::pixels holds before WriteImage),
 * other ranks' buffers are unspecified.  Blocks until `stream` is done.
 * Errors are collective-safe: a rank whose own arguments or state are unusable still takes part in the first (count)
 * exchange and reports the failure through it, so EVERY rank returns an error and none waits for a peer that left;
 * an error of the reduce or inside the send / recv group is returned only after the group is closed. */
int hprt_film_gather(HprtComm *c, HprtScene *s, float *d_film_xyzw, size_t n_pixels, int root, void *stream);
/* The same for ONE process that drives n GPUs with one HprtScene each (how an adapter inside pbrt would: the proposal
 * of SURVEY.md §8(b)); communicators come from ncclCommInitAll on first use.  d_films may be NULL (every scene's own film). */
int hprt_film_gather_local(HprtScene *const *per_gpu, float *const *d_films, int n, size_t n_pixels, int root);
/* Destroys the communicators hprt_film_gather_local created (ncclCommDestroy) and frees its staging buffers.  Call it
 * before the process ends while the HIP runtime is still alive; the library never does so from a static destructor. */
void hprt_film_gather_local_shutdown(void);
/* The transport-free halves, for hosts that move the data themselves (the gloo rehearsals in tests/ do): the records of
 * the last HPRT_RENDER_EXPORT_FOREIGN render (out == NULL: count only), and the ordered merge of any ranks' records into
 * a HOST copy of the summed films (sorts `records` by destination pixel and source tile, then adds; no GPU involved). */
typedef struct HprtFilmRecord {
    uint32_t dest_pixel;             /* row-major index into the cropped film */
    uint32_t src_tile;               /* tile (core/integrator.cpp:237-244 grid) whose samples these are */
    float xyz[3], weight;            /* that FilmTile pixel's contribSum as XYZ and its filterWeightSum */
} HprtFilmRecord;
int hprt_film_records_read(HprtScene *s, HprtFilmRecord *out, size_t capacity, size_t *n_records);
int hprt_film_records_merge(float *xyzw, size_t n_pixels, HprtFilmRecord *records, size_t n_records);

/* Radiance of individual camera samples (pixel x, y, sample index), after the
 * NaN/negative/inf guards of core/integrator.cpp:300-321; L_out = 3*n floats.
 * Test hook for per-sample parity. */
int hprt_sample_radiance(HprtScene *s, const HprtRenderOptions *opt, size_t n, const int32_t *px, const int32_t *py,
                         const int64_t *sample, float *L_out);

/* ------------------------------------------------------------------------ */
/* Integrator "ambientocclusion" (core/api.cpp:1922).  SamplerIntegrator::Render */
/* (core/integrator.cpp:230-360) with AOIntegrator::Li (integrators/ao.cpp:57-103) */
/* as the estimator: one closest hit per camera sample, then n_samples         */
/* hemisphere rays from the hit, each answered by Scene::IntersectP            */
/* (tMax = Infinity), drawn from the sampler's 2D array (Request2DArray,       */
/* ao.cpp:54; GlobalSampler::StartPixel, core/sampler.cpp:136-166: dimensions  */
/* 5 and 6 at index GetIndexForSample(pixel sample * n_samples + i)).  The     */
/* hemisphere rays go through the scene's walk — the BVH or an attached tree — */
/* never through the shadow grid.                                              */
/* Same film, tiles, spp_chunk, d_film_xyzw, stream and stats contract as      */
/* hprt_render (shadow_rays: the hemisphere rays, n_samples per camera ray     */
/* that hit); opt.max_depth / rr_threshold / light_strategy are not read.      */
/* Refused: n_samples outside 1..1024 (HPRT_E_INVALID), n_samples * spp above  */
/* INT32_MAX (the reference's int nSamples = size * samplesPerPixel overflows, */
/* core/sampler.cpp:157: HPRT_E_UNSUPPORTED), any flag but                     */
/* HPRT_RENDER_COUNT_WORK (HPRT_E_UNSUPPORTED).                                */
/* ------------------------------------------------------------------------ */
int hprt_render_ao(HprtScene *s, const HprtRenderDesc *desc, const HprtAoParams *ao, float *d_film_xyzw, void *stream,
                   HprtRenderStats *stats);
/* L (ao.cpp:57-103) of individual camera samples after the guards of core/integrator.cpp:300-321; L3_out = 3*n floats.
 * The AO twin of hprt_sample_radiance. */
int hprt_sample_ao(HprtScene *s, const HprtRenderOptions *opt, const HprtAoParams *ao, size_t n, const int32_t *px,
                   const int32_t *py, const int64_t *sample, float *L3_out);

/* ------------------------------------------------------------------------ */
/* Integrator "directlighting" (core/api.cpp:1913).  SamplerIntegrator::Render */
/* with DirectLightingIntegrator::Li (integrators/directlighting.cpp:62-100) as */
/* the estimator: at every hit isect.Le(wo), then UniformSampleAllLights over   */
/* the sampler's 2D arrays (two of n_light_samples[j] entries per light j and  */
/* depth, Preprocess :45-60; dimensions 5 .. 5 + 4 max_depth n_lights - 1, the */
/* plain dimensions follow; a node that finds the arrays used up takes one      */
/* sample per light from plain dimensions, core/integrator.cpp:67-72) or       */
/* UniformSampleOneLight (uniform pick), each through EstimateDirect; then,    */
/* while depth + 1 < max_depth, SpecularReflect and SpecularTransmit           */
/* (core/integrator.cpp:362-450) through mirror, uber and smooth-glass lobes   */
/* (GlassMaterial without allowMultipleLobes: two specular lobes).  An escaped  */
/* ray picks up every infinite light's Le.  All rays go through the scene's    */
/* walk - the BVH or an attached tree - never through the shadow grid.         */
/* n_light_samples: n_lights counts as hprt_model_direct reports them; NULL:   */
/* all 1.  Same film, tiles, spp_chunk, d_film_xyzw, stream and stats contract */
/* as hprt_render (rays: the node rays and EstimateDirect's BSDF-sampled rays; */
/* shadow_rays: its visibility rays); opt.max_depth / rr_threshold /           */
/* light_strategy are not read.                                                */
/* Refused before the device is touched - HPRT_E_INVALID: max_depth < 1, a     */
/* count < 1, n_lights other than the scene's; HPRT_E_UNSUPPORTED: max_depth   */
/* above HPRT_DIRECT_MAX_DEPTH; a tree whose worst case could pass the         */
/* reference's 1,000 Halton dimensions (5 + 4 max_depth n_lights for the       */
/* arrays, then per node of a full binary tree of max_depth levels its plain   */
/* light dimensions and, above the last level, 4 for the two specular calls);  */
/* a count * spp above INT32_MAX (core/sampler.cpp:157); more than 65,536      */
/* light samples per node; any flag but HPRT_RENDER_COUNT_WORK; and, with      */
/* max_depth > 1, a scene that holds an image texture and a material with a    */
/* specular lobe the recursion can follow (mirror; smooth glass; uber with     */
/* non-black Kr or Kt or an opacity that is textured or not 1): the reference  */
/* carries ray differentials through specular bounces, hprt does not.          */
/* ------------------------------------------------------------------------ */
int hprt_render_direct(HprtScene *s, const HprtRenderDesc *desc, const HprtDirectParams *params,
                       const int32_t *n_light_samples, size_t n_lights, float *d_film_xyzw, void *stream,
                       HprtRenderStats *stats);
/* L (directlighting.cpp:62-100) of individual camera samples after the guards of core/integrator.cpp:300-321; L3_out =
 * 3*n floats.  The twin of hprt_sample_ao. */
int hprt_sample_direct(HprtScene *s, const HprtRenderOptions *opt, const HprtDirectParams *params,
                       const int32_t *n_light_samples, size_t n_lights, size_t n, const int32_t *px, const int32_t *py,
                       const int64_t *sample, float *L3_out);

/* Halton sampler tables (host): ComputeRadicalInversePermutations
 * (core/lowdiscrepancy.cpp:2490-2504) with the default-seeded PCG32. */
int hprt_halton_permutations(uint16_t *out, size_t max_entries, size_t *n_entries);

#ifdef __cplusplus
}
#endif
#endif /* HPRT_H */
