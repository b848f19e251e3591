// hprt — BuildSceneLayout (scene_layout.h): the host half of hprt_scene_create, one stage per part of the HBM scene.  Built by
// hipcc as host code only (no offload target, no code object): the host code generator that compiled these float operations
// when they sat in capi_device.hip.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <utility>
#include "scene_layout.h"
#include "bvh_builder.h"
#include "device/dev_intersect.h"
#include "hprt_internal.h"
#include "wide_bvh.h"

namespace hprt {
namespace {

// TrowbridgeReitzDistribution::RoughnessToAlpha, core/microfacet.h:123-128 (host libm logf,
// as in the reference; constant textures make it a per-material constant)
float RoughnessToAlpha(float roughness) {
    roughness = sel_max(roughness, (float)1e-3);
    float x = std::log(roughness);
    return 1.62142f + 0.819955f * x + 0.1734f * x * x + 0.0171201f * x * x * x + 0.000640711f * x * x * x * x;
}

// Would Triangle::Intersect reject every hit on this triangle as "bogus"
// (shapes/triangle.cpp:300-316)?  Depends on the triangle only, so decided here.
bool TriangleIsBogus(vec3 p0, vec3 p1, vec3 p2, const float *uv0, const float *uv1, const float *uv2) {
    float u0x = 0, u0y = 0, u1x = 1, u1y = 0, u2x = 1, u2y = 1;
    if (uv0) { u0x = uv0[0]; u0y = uv0[1]; u1x = uv1[0]; u1y = uv1[1]; u2x = uv2[0]; u2y = uv2[1]; }
    float duv02x = u0x - u2x, duv02y = u0y - u2y, duv12x = u1x - u2x, duv12y = u1y - u2y;
    vec3 dp02 = p0 - p2, dp12 = p1 - p2;
    float determinant = duv02x * duv12y - duv02y * duv12x;
    bool degenerateUV = std::fabs(determinant) < 1e-8;
    vec3 dpdu, dpdv;
    if (!degenerateUV) {
        float invdet = 1 / determinant;
        dpdu = (duv12y * dp02 - duv02y * dp12) * invdet;
        dpdv = (-duv12x * dp02 + duv02x * dp12) * invdet;
    }
    if (degenerateUV || length2(cross(dpdu, dpdv)) == 0) {
        vec3 ng = cross(p2 - p0, p1 - p0);
        if (length2(ng) == 0) return true;
    }
    return false;
}

// MIPMap<RGBSpectrum>::Lookup(st, width) on the host, over an HprtTextureDesc (core/mipmap.h:203-260; repeat wrap): the same
// float operations as the device's mip_triangle / the oracle's MipLookupWidth.  Used once per infinite light for the scalar image
// of its Distribution2D (lights/infinite.cpp:66-85) and for Power() (:87-91).
inline int HostModI(int a, int b) { const int r = a - (a / b) * b; return r < 0 ? r + b : r; }
inline rgb HostMipTexel(const HprtTextureDesc &tx, int level, int s, int t) {
    const HprtTextureLevel &l = tx.levels[level];
    s = HostModI(s, l.w); t = HostModI(t, l.h);
    const float *p = l.rgb + 3 * ((size_t)t * (size_t)l.w + (size_t)s);
    return rgb(p[0], p[1], p[2]);
}
inline rgb HostMipTriangle(const HprtTextureDesc &tx, int level, float su, float sv) {
    level = level < 0 ? 0 : (level > (int)tx.n_levels - 1 ? (int)tx.n_levels - 1 : level);
    const HprtTextureLevel &l = tx.levels[level];
    const float s = su * l.w - 0.5f, t = sv * l.h - 0.5f;
    const int s0 = (int)std::floor(s), t0 = (int)std::floor(t);
    const float ds = s - s0, dt = t - t0;
    return (1 - ds) * (1 - dt) * HostMipTexel(tx, level, s0, t0) + (1 - ds) * dt * HostMipTexel(tx, level, s0, t0 + 1) +
           ds * (1 - dt) * HostMipTexel(tx, level, s0 + 1, t0) + ds * dt * HostMipTexel(tx, level, s0 + 1, t0 + 1);
}
inline rgb HostMipLookupWidth(const HprtTextureDesc &tx, float su, float sv, float width) {
    const int nLevels = (int)tx.n_levels;
    const float invLog2 = 1.442695040888963387004650940071;
    const float level = nLevels - 1 + det_logf(sel_max(width, (float)1e-8)) * invLog2;
    if (level < 0) return HostMipTriangle(tx, 0, su, sv);
    else if (level >= nLevels - 1) return HostMipTexel(tx, nLevels - 1, 0, 0);
    const int iLevel = (int)std::floor(level);
    const float delta = level - iLevel;
    return (1 - delta) * HostMipTriangle(tx, iLevel, su, sv) + delta * HostMipTriangle(tx, iLevel + 1, su, sv);
}

bool Textured(const HprtMaterialDesc &md) { return md.kd_texture >= 0 || md.ks_texture >= 0 || (md.type == 6 && md.opacity_texture >= 0); }

// ---- what the stages share ----
struct AggPrim { int32_t shape; uint32_t local; };      // shape < 0: instance `local`
// an aggregate: 0 = the top level (renderOptions->primitives), 1 + k = object definition k
struct Agg { const BvhNode *nodes; uint32_t nNodes; const uint32_t *order; uint32_t nPrims; std::vector<AggPrim> prims; };
struct Work {
    const HprtSceneDesc &d;
    SceneLayout &L;
    std::vector<uint64_t> vtxBase;          // per shape: its first vertex in vUV / vS (n_shapes + 1 entries)
    std::vector<uint32_t> shapePrims;       // per shape: its primitives
    std::vector<Agg> aggs;
    std::vector<uint32_t> primBase, pairBase;      // per aggregate (+ the total): its first primitive record and node pair
    std::vector<int> sphereOfShape;
    std::vector<int32_t> lightPrim;         // triangle lights: ordered index of their triangle
    std::vector<int32_t> wideBase;          // first wide record of every aggregate that has a tree
    uint32_t inlineMaterialMax;             // largest material index a triangle's tag carries (TAG_SHAPE_INLINE)
};

int ValidateArrays(Work &w) {
    const HprtSceneDesc *d = &w.d;
    if ((d->n_nodes && !d->nodes) || (d->n_prims && !d->prim_order) || (d->n_shapes && !d->shapes) ||
        (d->n_materials && !d->materials) || (d->n_lights && !d->lights))
        return SetError(HPRT_E_INVALID, "hprt_scene_create: null array with non-zero count");
    if (d->n_textures && !d->textures) return SetError(HPRT_E_INVALID, "hprt_scene_create: null texture array with non-zero count");
    if ((d->n_objects && !d->objects) || (d->n_instances && !d->instances) || (d->n_top && !d->top))
        return SetError(HPRT_E_INVALID, "hprt_scene_create: null instancing array with non-zero count");
    return HPRT_OK;
}

int ValidateShapes(Work &w) {
    const HprtSceneDesc *d = &w.d;
    w.vtxBase.assign(d->n_shapes + 1, 0);
    w.shapePrims.assign(d->n_shapes, 0);
    for (uint32_t s = 0; s < d->n_shapes; ++s) {
        const HprtShapeDesc &sh = d->shapes[s];
        if (sh.material < 0 || (uint32_t)sh.material >= d->n_materials) return SetError(HPRT_E_INVALID, "shape material index out of range");
        if (sh.area_light >= (int32_t)d->n_lights) return SetError(HPRT_E_INVALID, "shape area light index out of range");
        if (sh.kind == 0) {
            if (sh.n_tris && (!sh.indices || !sh.P)) return SetError(HPRT_E_INVALID, "mesh without indices or positions");
            for (uint64_t i = 0; i < 3ull * sh.n_tris; ++i)
                if (sh.indices[i] < 0 || (uint32_t)sh.indices[i] >= sh.n_verts) return SetError(HPRT_E_INVALID, "mesh vertex index out of range");
            // an emissive mesh owns one light per triangle, consecutive and in face order (core/api.cpp:1609-1636)
            if (sh.area_light >= 0) {
                if ((uint64_t)sh.area_light + sh.n_tris > d->n_lights) return SetError(HPRT_E_INVALID, "emissive mesh: its per-triangle lights exceed the light table");
                for (uint32_t t = 0; t < sh.n_tris; ++t)
                    if (d->lights[sh.area_light + t].type != 2 || d->lights[sh.area_light + t].shape != (int32_t)s)
                        return SetError(HPRT_E_INVALID, "emissive mesh: light area_light + t must be the diffuse area light of its triangle t");
            }
            w.shapePrims[s] = sh.n_tris; w.vtxBase[s + 1] = w.vtxBase[s] + sh.n_verts;
        } else if (sh.kind == 1) {
            w.shapePrims[s] = 1; w.vtxBase[s + 1] = w.vtxBase[s];
        } else return SetError(HPRT_E_INVALID, "unknown shape kind");
    }
    if (w.vtxBase[d->n_shapes] > 0xffffffffull) return SetError(HPRT_E_UNSUPPORTED, "more than 2^32 vertices");
    return HPRT_OK;
}

int GatherAggregates(Work &w) {
    const HprtSceneDesc *d = &w.d;
    std::vector<Agg> &aggs = w.aggs;
    aggs.resize(1 + (size_t)d->n_objects);
    std::vector<int32_t> objectOfShape(d->n_shapes, -1);
    aggs[0].nodes = (const BvhNode *)d->nodes; aggs[0].nNodes = d->n_nodes; aggs[0].order = d->prim_order; aggs[0].nPrims = d->n_prims;
    auto addShape = [&](Agg &a, uint32_t s) { for (uint32_t k = 0; k < w.shapePrims[s]; ++k) a.prims.push_back(AggPrim{(int32_t)s, k}); };
    for (uint32_t k = 0; k < d->n_objects; ++k) {
        const HprtObjectDesc &o = d->objects[k];
        Agg &a = aggs[1 + (size_t)k];
        if ((uint64_t)o.first_shape + o.n_shapes > d->n_shapes) return SetError(HPRT_E_INVALID, "object shape range out of bounds");
        if ((o.n_nodes && !o.nodes) || (o.n_prims && !o.prim_order)) return SetError(HPRT_E_INVALID, "object without its aggregate arrays");
        a.nodes = (const BvhNode *)o.nodes; a.nNodes = o.n_nodes; a.order = o.prim_order; a.nPrims = o.n_prims;
        for (uint32_t s = o.first_shape; s < o.first_shape + o.n_shapes; ++s) {
            if (objectOfShape[s] >= 0) return SetError(HPRT_E_INVALID, "a shape belongs to two objects");
            if (d->shapes[s].area_light >= 0) return SetError(HPRT_E_UNSUPPORTED, "area lights are not supported with object instancing (core/api.cpp:1640)");
            objectOfShape[s] = (int32_t)k;
            addShape(a, s);
        }
    }
    for (uint32_t i = 0; i < d->n_instances; ++i) {
        const int32_t o = d->instances[i].object;
        if (o < 0 || (uint32_t)o >= d->n_objects) return SetError(HPRT_E_INVALID, "instance object index out of range");
        if (aggs[1 + (size_t)o].prims.empty()) return SetError(HPRT_E_INVALID, "instance of an empty object");
    }
    if (d->top) {
        for (uint32_t t = 0; t < d->n_top; ++t) {
            const HprtTopItem &it = d->top[t];
            if (it.kind == 0) {
                if (it.index >= d->n_shapes || objectOfShape[it.index] >= 0) return SetError(HPRT_E_INVALID, "top-level item references a missing or object-owned shape");
                addShape(aggs[0], it.index);
            } else if (it.kind == 1) {
                if (it.index >= d->n_instances) return SetError(HPRT_E_INVALID, "top-level item references a missing instance");
                aggs[0].prims.push_back(AggPrim{-1, it.index});
            } else return SetError(HPRT_E_INVALID, "unknown top-level item kind");
        }
    } else {
        if (d->n_instances) return SetError(HPRT_E_INVALID, "instances need the top-level item list");
        for (uint32_t s = 0; s < d->n_shapes; ++s) if (objectOfShape[s] < 0) addShape(aggs[0], s);
    }
    return HPRT_OK;
}

// Each aggregate's tree and primitive order, and where its records start in the shared arrays (32-bit byte offsets address them)
int CheckAggregates(Work &w) {
    const size_t nAggs = w.aggs.size();
    w.primBase.assign(nAggs + 1, 0); w.pairBase.assign(nAggs + 1, 0);
    uint64_t np = 0, npair = 0;
    int topDepth = 0, objectDepth = 0;
    for (size_t a = 0; a < nAggs; ++a) {
        const Agg &g = w.aggs[a];
        if (g.prims.size() != g.nPrims) return SetError(HPRT_E_INVALID, "prim_order length does not match the aggregate's primitive count");
        int depth = 0;
        const char *bad = CheckBvhNodes(g.nodes, g.nNodes, g.nPrims, &depth);
        if (*bad) return SetError(HPRT_E_INVALID, bad);
        if ((g.nPrims != 0) != (g.nNodes != 0)) return SetError(HPRT_E_INVALID, "aggregate with primitives but no nodes (or the reverse)");
        for (uint32_t i = 0; i < g.nPrims; ++i) if (g.order[i] >= g.nPrims) return SetError(HPRT_E_INVALID, "prim_order entry out of range");
        uint32_t interior = 0;
        for (uint32_t i = 0; i < g.nNodes; ++i) interior += (g.nodes[i].countAxis & 3u) != 3u;
        w.primBase[a] = (uint32_t)np; w.pairBase[a] = (uint32_t)npair;
        np += g.nPrims; npair += g.nNodes ? interior + 1u : 0u;
        if (np * 48ull > 0xffffffffull || npair * 64ull > 0xffffffffull)
            return SetError(HPRT_E_UNSUPPORTED, "more than 89,478,485 primitives (or 67,108,863 interior nodes) over all aggregates");
        if (a == 0) topDepth = depth; else objectDepth = std::max(objectDepth, depth);
    }
    w.primBase[nAggs] = (uint32_t)np; w.pairBase[nAggs] = (uint32_t)npair;
    // The ordered walk keeps at most one pending sibling per level, plus the sentinel of an instance: the kernel's
    // stack has HPRT_STACK_TOTAL = 64 entries (LDS + HBM part), as the reference's nodesToVisit[64]
    // (accelerators/bvh.cpp:365).  Deeper trees are refused here rather than walked wrongly.
    if (topDepth + (w.d.n_instances ? 1 + objectDepth : 0) > HPRT_STACK_TOTAL)
        return SetError(HPRT_E_UNSUPPORTED, "BVH deeper than the 64-entry traversal stack (accelerators/bvh.cpp:365 reserves the same)");
    return HPRT_OK;
}

int ValidateLights(Work &w) {
    const HprtSceneDesc *d = &w.d;
    for (uint32_t l = 0; l < d->n_lights; ++l) {
        const HprtLightDesc &L = d->lights[l];
        if (L.type < 0 || L.type > 3) return SetError(HPRT_E_INVALID, "unknown light type");
        if (L.type == 3) {
            if (L.texture < 0 || (uint32_t)L.texture >= d->n_textures) return SetError(HPRT_E_INVALID, "infinite light: map index out of range");
            const HprtTextureDesc &mt = d->textures[L.texture];
            if (!mt.levels || mt.n_levels == 0 || mt.n_levels > 26 || mt.wrap != 0) return SetError(HPRT_E_INVALID, "infinite light: its map must be a repeat-wrapped pyramid of at most 26 levels");
            if ((uint64_t)mt.levels[0].w * (uint64_t)mt.levels[0].h > (1ull << 26)) return SetError(HPRT_E_UNSUPPORTED, "infinite light: map larger than 2^26 texels");
        }
        if (L.type == 2) {
            if (L.shape < 0 || (uint32_t)L.shape >= d->n_shapes) return SetError(HPRT_E_INVALID, "area light shape out of range");
            const HprtShapeDesc &ls = d->shapes[L.shape];
            const bool own = ls.kind == 1 ? ls.area_light == (int32_t)l
                                          : ls.area_light >= 0 && (int32_t)l >= ls.area_light && (uint32_t)((int32_t)l - ls.area_light) < ls.n_tris;
            if (!own) return SetError(HPRT_E_INVALID, "area light and its shape do not reference each other");
        }
    }
    // CreateLightSampleDistribution (core/lightdistrib.cpp:48-66): a single light always gets the uniform distribution
    w.L.lightStrategy = d->n_lights <= 1 ? 0 : d->light_strategy;
    if (w.L.lightStrategy < 0 || w.L.lightStrategy > 2) return SetError(HPRT_E_INVALID, "light_strategy must be 0 (uniform), 1 (power) or 2 (spatial)");
    return HPRT_OK;
}

// Shapes, spheres and the per-vertex shading attributes
int LayoutShapes(Work &w) {
    const HprtSceneDesc *d = &w.d;
    SceneLayout &L = w.L;
    const uint32_t nVtx = (uint32_t)w.vtxBase[d->n_shapes];
    L.vUV.assign(2 * (size_t)nVtx, 0.f); L.vS.assign(3 * (size_t)nVtx, 0.f);
    L.shapes.resize(d->n_shapes);
    w.sphereOfShape.assign(d->n_shapes, -1);
    for (uint32_t s = 0; s < d->n_shapes; ++s) {
        const HprtShapeDesc &sh = d->shapes[s];
        DevShape &o = L.shapes[s];
        o.material = sh.material; o.areaLight = sh.area_light; o.sphere = -1;
        o.flags = ((sh.reverse_orientation != 0) ^ (sh.transform_swaps_handedness != 0)) ? SHAPE_FLIP : 0u;
        if (sh.reverse_orientation) o.flags |= SHAPE_REVERSE;
        if (sh.kind == 0) {
            size_t b = w.vtxBase[s];
            if (sh.N) o.flags |= SHAPE_HAS_N;
            if (sh.UV) { o.flags |= SHAPE_HAS_UV; memcpy(&L.vUV[2 * b], sh.UV, 8 * (size_t)sh.n_verts); }
            if (sh.S) { o.flags |= SHAPE_HAS_S; memcpy(&L.vS[3 * b], sh.S, 12 * (size_t)sh.n_verts); }
        } else {
            DevSphere sp;
            memcpy(sp.o2w.m, sh.object_to_world, 64); memcpy(sp.w2o.m, sh.world_to_object, 64);
            sp.radius = sh.radius; sp.zMin = sh.z_min; sp.zMax = sh.z_max; sp.thetaMin = sh.theta_min; sp.thetaMax = sh.theta_max; sp.phiMax = sh.phi_max;
            o.sphere = w.sphereOfShape[s] = (int)L.spheres.size();
            L.spheres.push_back(sp);
        }
    }
    return HPRT_OK;
}

// The 48-byte primitive records of every aggregate in BVH order, with their shading bins, vertex ids and shading normals
int LayoutPrimitives(Work &w) {
    const HprtSceneDesc *d = &w.d;
    SceneLayout &L = w.L;
    const size_t n = 3 * (size_t)L.nPrims;
    L.tris.resize(n); L.primVtx.assign(n, 0u); L.primN.assign(n, make_float4(0.f, 0.f, 0.f, 0.f));
    w.lightPrim.assign(d->n_lights, -1);
    for (size_t ai = 0; ai < w.aggs.size(); ++ai) {
        const Agg &g = w.aggs[ai];
        for (uint32_t oi = 0; oi < g.nPrims; ++oi) {
            const size_t i = (size_t)w.primBase[ai] + oi;
            const AggPrim e = g.prims[g.order[oi]];
            float4 r0, r1, r2;
            if (e.shape < 0) {     // TransformedPrimitive
                r0 = make_float4(0, 0, 0, u2f(TAG_INSTANCE)); r1 = make_float4(0, 0, 0, u2f(0u)); r2 = make_float4(0, 0, 0, u2f(e.local));
            } else {
                const uint32_t s = (uint32_t)e.shape;
                const HprtShapeDesc &sh = d->shapes[s];
                const HprtMaterialDesc &md = d->materials[sh.material];
                if (sh.kind == 0) {
                    const int32_t *v = &sh.indices[3 * (size_t)e.local];
                    const float *a = &sh.P[3 * (size_t)v[0]], *b = &sh.P[3 * (size_t)v[1]], *c = &sh.P[3 * (size_t)v[2]];
                    bool bogus = TriangleIsBogus(vec3(a[0], a[1], a[2]), vec3(b[0], b[1], b[2]), vec3(c[0], c[1], c[2]),
                                                 sh.UV ? &sh.UV[2 * (size_t)v[0]] : nullptr, sh.UV ? &sh.UV[2 * (size_t)v[1]] : nullptr,
                                                 sh.UV ? &sh.UV[2 * (size_t)v[2]] : nullptr);
                    // a triangle of an emissive mesh: aux = 1 + its light, and TAG_GENERIC — the generic shading variant is the one that looks for Le
                    const int32_t triLight = sh.area_light >= 0 ? sh.area_light + (int32_t)e.local : -1;
                    if (triLight >= 0) w.lightPrim[triLight] = (int32_t)i;
                    // the shading bin: plain matte / plastic / substrate triangles have kernels of their own; emitters, textured and every other
                    // material (OrenNayar, mirror, metal, glass, uber) are shaded by the generic variant
                    const uint32_t bin = Textured(md) ? BIN_TEXTURED : triLight >= 0 ? BIN_GENERIC : md.type == 1 ? BIN_PLASTIC : md.type == 3 ? BIN_SUBSTRATE :
                                         (md.type == 0 && clampf(md.sigma, 0.f, 90.f) == 0.f) ? BIN_MATTE : BIN_GENERIC;
                    uint32_t tag = (bogus ? TAG_BOGUS : 0u) | (bin << TAG_BIN_SHIFT);
                    // what shading reads of shapes[s] travels in the tag when the material index fits (dev_scene.h)
                    if ((uint32_t)sh.material <= w.inlineMaterialMax)
                        tag |= TAG_SHAPE_INLINE | ((L.shapes[s].flags & SHAPE_FLAGS_MASK) << TAG_SHAPE_FLAGS_SHIFT) | ((uint32_t)sh.material << TAG_MATERIAL_SHIFT);
                    if (bin == BIN_SUBSTRATE) L.hasSubstrateBin = true;
                    r0 = make_float4(a[0], a[1], a[2], u2f(tag)); r1 = make_float4(b[0], b[1], b[2], u2f(s)); r2 = make_float4(c[0], c[1], c[2], u2f((uint32_t)(triLight + 1)));
                    for (int k = 0; k < 3; ++k) {
                        L.primVtx[3 * i + k] = (uint32_t)(w.vtxBase[s] + (uint32_t)v[k]);
                        if (sh.N) { const float *nn = &sh.N[3 * (size_t)v[k]]; L.primN[3 * i + k] = make_float4(nn[0], nn[1], nn[2], 0.f); }
                    }
                } else {
                    r0 = make_float4(0, 0, 0, u2f(TAG_SPHERE | ((Textured(md) ? BIN_TEXTURED : BIN_GENERIC) << TAG_BIN_SHIFT))); r1 = make_float4(0, 0, 0, u2f(s)); r2 = make_float4(0, 0, 0, u2f((uint32_t)w.sphereOfShape[s]));
                }
            }
            L.tris[3 * i] = r0; L.tris[3 * i + 1] = r1; L.tris[3 * i + 2] = r2;
        }
    }
    return HPRT_OK;
}

int LayoutMaterials(Work &w) {
    const HprtSceneDesc *d = &w.d;
    w.L.materials.resize(d->n_materials);
    for (uint32_t m = 0; m < d->n_materials; ++m) {
        const HprtMaterialDesc &in = d->materials[m];
        if (in.type < 0 || in.type > 6) return SetError(HPRT_E_UNSUPPORTED, "material type outside the hot-path scope (matte, plastic, mirror, substrate, metal, glass, uber)");
        if (in.kd_texture >= (int32_t)d->n_textures || in.ks_texture >= (int32_t)d->n_textures || (in.type == 6 && in.opacity_texture >= (int32_t)d->n_textures))
            return SetError(HPRT_E_INVALID, "material texture index out of range");
        DevMaterial &o = w.L.materials[m];
        o.KdTex = in.kd_texture >= 0 ? in.kd_texture : -1; o.KsTex = in.ks_texture >= 0 ? in.ks_texture : -1;
        o.opTex = in.type == 6 && in.opacity_texture >= 0 ? in.opacity_texture : -1;
        o.type = in.type; memcpy(o.Kd, in.Kd, 12); memcpy(o.Ks, in.Ks, 12);
        o.alpha = in.remap_roughness ? RoughnessToAlpha(in.roughness) : in.roughness;
        o.alphaY = o.alpha;
        if (in.type == 3 || in.type == 4 || in.type == 6) o.alphaY = in.remap_roughness ? RoughnessToAlpha(in.sigma) : in.sigma;      // substrate / metal / uber: sigma carries vroughness
        memcpy(o.Kr, in.Kr, 12); memcpy(o.Kt, in.Kt, 12); memcpy(o.opacity, in.opacity, 12); o.eta = in.eta;
        o.roughGlass = 0;
        if (in.type == 5) {
            o.alpha = in.roughness;      // glass: the index of refraction, as given
            // rough dielectric (materials/glass.cpp:61-72): isSpecular is decided on the values as given, the remap applies to both after it
            if (in.sigma != 0.f || in.Kr[0] != 0.f) {
                o.roughGlass = 1;
                o.Kr[0] = in.remap_roughness ? RoughnessToAlpha(in.sigma) : in.sigma;
                o.Kr[1] = in.remap_roughness ? RoughnessToAlpha(in.Kr[0]) : in.Kr[0];
            }
        }
        // MatteMaterial: sig = Clamp(sigma, 0, 90); sig != 0 -> OrenNayar(r, sig) (materials/matte.cpp:55-61, core/reflection.h:414-420)
        const float sig = clampf(in.sigma, 0.f, 90.f);
        o.oren = in.type == 0 && sig != 0.f ? 1 : 0; o.orenA = 1.f; o.orenB = 0.f;
        if (o.oren) {
            const float sigma = (HPRT_PI / 180) * sig;
            const float sigma2 = sigma * sigma;
            o.orenA = 1.f - (sigma2 / (2.f * (sigma2 + 0.33f)));
            o.orenB = 0.45f * sigma2 / (sigma2 + 0.09f);
        }
    }
    return HPRT_OK;
}

// Image textures: every pyramid level of every texture in one texel array (3 floats per texel)
int LayoutTextures(Work &w) {
    const HprtSceneDesc *d = &w.d;
    SceneLayout &L = w.L;
    L.textures.resize(d->n_textures);
    for (uint32_t t = 0; t < d->n_textures; ++t) {
        const HprtTextureDesc &in = d->textures[t];
        if (!in.levels || in.n_levels == 0 || in.n_levels > 32 || !in.weight_lut) return SetError(HPRT_E_INVALID, "texture without levels or weight table");
        if (in.wrap < 0 || in.wrap > 2) return SetError(HPRT_E_INVALID, "texture wrap mode out of range");
        DevTexture &o = L.textures[t];
        o.firstLevel = (uint32_t)L.mipLevels.size(); o.nLevels = in.n_levels; o.trilinear = in.trilinear ? 1 : 0; o.wrap = in.wrap;
        o.maxAniso = in.max_anisotropy; o.su = in.su; o.sv = in.sv; o.du = in.du; o.dv = in.dv;
        for (uint32_t l = 0; l < in.n_levels; ++l) {
            const HprtTextureLevel &lv = in.levels[l];
            if (lv.w <= 0 || lv.h <= 0 || !lv.rgb) return SetError(HPRT_E_INVALID, "empty texture level");
            const size_t n = 3 * (size_t)lv.w * (size_t)lv.h;
            if (L.texels.size() + n > 0xffffffffull) return SetError(HPRT_E_UNSUPPORTED, "more than 2^32 texture floats");
            L.mipLevels.push_back(DevMipLevel{(uint32_t)L.texels.size(), lv.w, lv.h});
            L.texels.insert(L.texels.end(), lv.rgb, lv.rgb + n);
        }
        // MIPMap::weightLut is a static table (core/mipmap.h:107, 153-161): identical for every texture
        if (t == 0) L.weightLut.assign(in.weight_lut, in.weight_lut + 128);
        else if (memcmp(L.weightLut.data(), in.weight_lut, 128 * sizeof(float)) != 0) return SetError(HPRT_E_INVALID, "textures disagree on the EWA weight table");
    }
    return HPRT_OK;
}

int LayoutLights(Work &w) {
    const HprtSceneDesc *d = &w.d;
    w.L.lights.resize(d->n_lights);
    for (uint32_t l = 0; l < d->n_lights; ++l) {
        const HprtLightDesc &in = d->lights[l];
        DevLight &o = w.L.lights[l];
        o.type = in.type; memcpy(o.pos, in.pos, 12); memcpy(o.I, in.I, 12); o.shape = in.shape; o.twoSided = in.two_sided;
        const bool onMesh = in.type == 2 && d->shapes[in.shape].kind == 0;
        if (onMesh && w.lightPrim[l] < 0) return SetError(HPRT_E_UNSUPPORTED, "emissive triangle outside the top-level aggregate (area lights are not supported with object instancing, core/api.cpp:1640)");
        if (onMesh) o.type = 3;
        o.prim = onMesh ? w.lightPrim[l] : -1;
        o.sphere = in.type == 2 && !onMesh ? w.sphereOfShape[in.shape] : -1;
        o.shapeFlags = in.type == 2 ? w.L.shapes[in.shape].flags : 0u;
    }
    return HPRT_OK;
}

// Infinite lights: the scalar image of lights/infinite.cpp:66-85 (2w x 2h: luminance of the filtered map times sin theta) and
// its Distribution2D, built with the float operations of Distribution1D's constructor (hprt_math.h dist1d_build)
int LayoutEnvLights(Work &w) {
    const HprtSceneDesc *d = &w.d;
    SceneLayout &L = w.L;
    for (uint32_t l = 0; l < d->n_lights; ++l) {
        const HprtLightDesc &in = d->lights[l];
        if (in.type != 3) continue;
        const HprtTextureDesc &tx = d->textures[in.texture];
        DevEnvLight e; memset(&e, 0, sizeof(e));
        memcpy(&e.l2w, in.light_to_world, 64); memcpy(&e.w2l, in.world_to_light, 64);
        e.tex = in.texture;
        const int width = 2 * tx.levels[0].w, height = 2 * tx.levels[0].h;
        e.nu = width; e.nv = height; e.off = (uint32_t)L.envData.size();
        const size_t nFloats = (size_t)height * width + (size_t)height * (width + 1) + (size_t)height + (size_t)height + 1;
        if (L.envData.size() + nFloats > 0x7fffffffull) return SetError(HPRT_E_UNSUPPORTED, "infinite light maps too large");
        L.envData.resize(L.envData.size() + nFloats);
        float *condFunc = L.envData.data() + e.off, *condCdf = condFunc + (size_t)height * width, *condInt = condCdf + (size_t)height * (width + 1),
              *margCdf = condInt + height;
        const float fwidth = 0.5f / std::min(width, height);
        for (int v = 0; v < height; ++v) {
            const float vp = (v + .5f) / (float)height;
            const float sinTheta = det_sinf(HPRT_PI * (v + .5f) / height);
            for (int u = 0; u < width; ++u) {
                const float up = (u + .5f) / (float)width;
                float y = luminance(HostMipLookupWidth(tx, up, vp, fwidth));
                y *= sinTheta;
                condFunc[(size_t)v * width + u] = y;
            }
            dist1d_build(condFunc + (size_t)v * width, width, condCdf + (size_t)v * (width + 1), &condInt[v]);
        }
        dist1d_build(condInt, height, margCdf, &e.margFuncInt);
        DevLight &o = L.lights[l];
        o.type = 4; o.shape = (int32_t)L.envLights.size();
        L.envLights.push_back(e);
    }
    return HPRT_OK;
}

// The world bound, the light sampling distribution and the spatial strategy's voxel grid
int LayoutLightDistribution(Work &w) {
    const HprtSceneDesc *d = &w.d;
    SceneLayout &L = w.L;
    // Scene::worldBound + Bounds3::BoundingSphere (core/scene.h:56-66, core/geometry.h:980-983)
    vec3 wbLo, wbHi;
    if (d->n_nodes) {
        const BvhNode &root = ((const BvhNode *)d->nodes)[0];
        wbLo = vec3(root.bmin[0], root.bmin[1], root.bmin[2]); wbHi = vec3(root.bmax[0], root.bmax[1], root.bmax[2]);
        vec3 c = div_by(wbLo + wbHi, 2.f);
        bool inside = c.x >= wbLo.x && c.x <= wbHi.x && c.y >= wbLo.y && c.y <= wbHi.y && c.z >= wbLo.z && c.z <= wbHi.z;
        L.worldRadius = inside ? dist(c, wbHi) : 0.f;
    }
    for (int a = 0; a < 3; ++a) { L.wbMin[a] = wbLo.get(a); L.wbMax[a] = wbHi.get(a); }
    // UniformLightDistribution (core/lightdistrib.cpp:68-75) or PowerLightDistribution (:77-82, ComputeLightPowerDistribution,
    // core/integrator.cpp:219-227: Light::Power().y()) as a Distribution1D (core/sampling.h:57-70)
    L.lightFunc.assign(std::max<uint32_t>(1, d->n_lights), 1.f); L.lightCdf.assign(d->n_lights + 1, 0.f);
    if (L.lightStrategy == 1)
        for (uint32_t l = 0; l < d->n_lights; ++l) {
            const HprtLightDesc &in = d->lights[l];
            const rgb I(in.I[0], in.I[1], in.I[2]);
            rgb power;
            if (in.type == 0) power = I * (4 * HPRT_PI);                                      // lights/point.cpp:55
            else if (in.type == 1) power = I * HPRT_PI * L.worldRadius * L.worldRadius;      // lights/distant.cpp:61-63
            else if (in.type == 3) power = HPRT_PI * L.worldRadius * L.worldRadius * HostMipLookupWidth(d->textures[in.texture], .5f, .5f, .5f);   // lights/infinite.cpp:87-91
            else {                                                                            // lights/diffuse.cpp:64-66, area = shape->Area()
                const HprtShapeDesc &ls = d->shapes[in.shape];
                float area;
                if (ls.kind == 1) area = ls.phi_max * ls.radius * (ls.z_max - ls.z_min);      // Sphere::Area, shapes/sphere.cpp:215
                else {                                                                        // Triangle::Area, shapes/triangle.cpp:576-582
                    const int32_t *v = &ls.indices[3 * (size_t)((int32_t)l - ls.area_light)];
                    const vec3 p0(ls.P[3 * v[0]], ls.P[3 * v[0] + 1], ls.P[3 * v[0] + 2]), p1(ls.P[3 * v[1]], ls.P[3 * v[1] + 1], ls.P[3 * v[1] + 2]),
                               p2(ls.P[3 * v[2]], ls.P[3 * v[2] + 1], ls.P[3 * v[2] + 2]);
                    area = (float)(0.5 * (double)length(cross(p1 - p0, p2 - p0)));
                }
                power = I * (float)(in.two_sided ? 2 : 1) * area * HPRT_PI;
            }
            L.lightFunc[l] = luminance(power);
        }
    if (d->n_lights) dist1d_build(L.lightFunc.data(), (int)d->n_lights, L.lightCdf.data(), &L.funcInt);
    if (L.lightStrategy == 2) {
        // SpatialLightDistribution (core/lightdistrib.cpp:95-120, maxVoxels = 64): the voxel grid over the world bound
        const vec3 diag = wbHi - wbLo;
        const int me = (diag.x > diag.y && diag.x > diag.z) ? 0 : (diag.y > diag.z ? 1 : 2);      // Bounds3::MaximumExtent
        const float bmax = diag.get(me);
        for (int a = 0; a < 3; ++a) L.voxN[a] = std::max(1, int(std::round(diag.get(a) / bmax * 64)));
    }
    return HPRT_OK;
}

// The child-pair records of every aggregate's tree (device/dev_scene.h): one run of pairs per aggregate
int LayoutPairs(Work &w) {
    SceneLayout &L = w.L;
    L.pairs.resize((size_t)w.pairBase[w.aggs.size()]);
    for (size_t ai = 0; ai < w.aggs.size(); ++ai) {
        const Agg &g = w.aggs[ai];
        if (g.nNodes == 0) continue;
        const BvhNode *nd = g.nodes;
        std::vector<int32_t> ref(g.nNodes);
        int32_t nextPair = (int32_t)w.pairBase[ai] + 1;
        for (uint32_t i = 0; i < g.nNodes; ++i) {
            if ((nd[i].countAxis & 3u) == 3u) {
                ref[i] = ~(int32_t)(w.primBase[ai] + (uint32_t)nd[i].offset);
                const size_t last = (size_t)w.primBase[ai] + (uint32_t)nd[i].offset + (nd[i].countAxis >> 2) - 1u;
                L.tris[3 * last].w = u2f(f2u(L.tris[3 * last].w) | TAG_LAST);
            } else ref[i] = nextPair++;
        }
        auto fill = [&](DevPair &p, uint32_t c0, uint32_t c1, uint32_t meta) {
            const BvhNode &a = nd[c0], &b = nd[c1];
            p.x[0] = a.bmin[0]; p.x[1] = b.bmin[0]; p.x[2] = a.bmax[0]; p.x[3] = b.bmax[0];
            p.y[0] = a.bmin[1]; p.y[1] = b.bmin[1]; p.y[2] = a.bmax[1]; p.y[3] = b.bmax[1];
            p.z[0] = a.bmin[2]; p.z[1] = b.bmin[2]; p.z[2] = a.bmax[2]; p.z[3] = b.bmax[2];
            p.ref0 = ref[c0]; p.ref1 = ref[c1]; p.meta = meta; p.pad = 0u;
        };
        fill(L.pairs[w.pairBase[ai]], 0u, 0u, PAIR_SINGLE);      // synthetic parent of the root: carries the root's bounds test
        for (uint32_t i = 0; i < g.nNodes; ++i) {
            if ((nd[i].countAxis & 3u) == 3u) continue;
            fill(L.pairs[(size_t)ref[i]], i + 1u, (uint32_t)nd[i].offset, nd[i].countAxis & 3u);
        }
    }
    return HPRT_OK;
}

// The leaf-exact walk of plain renders (wide_bvh.h): four-wide records over the same leaves, for scenes without object instances.
// A leaf that holds exactly one triangle needs no stored box: Triangle::WorldBound is the min / max of its vertices
// (shapes/triangle.cpp:180-186) — provided that is, bit for bit, what the node holds (a zero of either sign among the
// coordinates would make the minimum's sign a matter of operand order: such leaves read their box like the others).
int LayoutWide(Work &w) {
    SceneLayout &L = w.L;
    w.wideBase.assign(w.aggs.size(), -1);
    bool wideOk = L.nPrims < (1u << 28);
    int wideNeedTop = 0, wideNeedObject = 0;
    for (size_t ai = 0; ai < w.aggs.size() && wideOk; ++ai) {
        const Agg &g = w.aggs[ai];
        if (g.nNodes == 0) continue;
        const BvhNode *nd = g.nodes;
        std::vector<int32_t> leafRefW(g.nNodes, WIDE_NONE);
        if (L.leafBox.empty()) { L.leafBox.assign(2 * (size_t)L.nPrims, make_float4(0.f, 0.f, 0.f, 0.f)); L.primSingle.assign(L.nPrims, 0); }
        for (uint32_t i = 0; i < g.nNodes; ++i) {
            if ((nd[i].countAxis & 3u) != 3u) continue;
            const uint32_t firstPrim = w.primBase[ai] + (uint32_t)nd[i].offset, count = nd[i].countAxis >> 2;
            bool single = count == 1u && (f2u(L.tris[3 * (size_t)firstPrim].w) & TAG_KIND_MASK) == 0u;
            if (single) {
                const float4 *v = &L.tris[3 * (size_t)firstPrim];
                const float c[3][3] = {{v[0].x, v[1].x, v[2].x}, {v[0].y, v[1].y, v[2].y}, {v[0].z, v[1].z, v[2].z}};
                for (int a = 0; a < 3 && single; ++a) {
                    bool posZero = false, negZero = false;
                    for (int k = 0; k < 3; ++k) { if (c[a][k] != c[a][k]) single = false; if (c[a][k] == 0.f) { if (f2u(c[a][k]) >> 31) negZero = true; else posZero = true; } }
                    const float mn = std::min(std::min(c[a][0], c[a][1]), c[a][2]), mx = std::max(std::max(c[a][0], c[a][1]), c[a][2]);
                    if ((posZero && negZero) || f2u(mn) != f2u(nd[i].bmin[a]) || f2u(mx) != f2u(nd[i].bmax[a])) single = false;
                }
            }
            uint32_t r = ~firstPrim;
            if (!single) r &= ~WIDE_LEAF_BOXED;
            else L.primSingle[firstPrim] = 1;
            leafRefW[i] = (int32_t)r;
            for (uint32_t k = 0; k < count; ++k) {
                L.leafBox[2 * (size_t)(firstPrim + k)] = make_float4(nd[i].bmin[0], nd[i].bmin[1], nd[i].bmin[2], nd[i].bmax[0]);
                L.leafBox[2 * (size_t)(firstPrim + k) + 1] = make_float4(nd[i].bmax[1], nd[i].bmax[2], 0.f, 0.f);
            }
        }
        int need = 0;
        w.wideBase[ai] = (int32_t)L.wide.size();
        if (!BuildWide(nd, g.nNodes, leafRefW.data(), &L.wide, &need)) wideOk = false;
        if (ai == 0) wideNeedTop = need; else wideNeedObject = std::max(wideNeedObject, need);
    }
    // (the wide walk's stack: LDS entries + the scene's deep-stack area; a scene that could need more keeps the binary walk)
    if (!wideOk || wideNeedTop + (w.d.n_instances ? 1 + wideNeedObject : 0) > HPRT_WIDE_STACK_MAX || w.wideBase[0] != 0) { L.wide.clear(); L.leafBox.clear(); L.primSingle.clear(); }
    return HPRT_OK;
}

// The shadow grid of a scene whose every shadow ray ends at one point (shadow_grid.h: exactly one light, a point light) or runs along
// one direction (distant_grid.h: exactly one light, a distant light, worldRadius > 0); triangles only, no object instances; the
// leaf-exact walk in use (its leaf boxes and one-triangle marks are what the grid kernels test with).
// HPRT_SHADOW_GRID=0: no grid (A/B runs); unset: only a grid that is expected to be cheaper than the walk (SG_MAX_CANDIDATES); 1: any.
// Everything else keeps the walk for its shadow rays.
int LayoutShadowGrid(Work &w) {
    SceneLayout &L = w.L;
    const int mode = ShadowGridModeFromEnv();
    if (mode == 0 || w.d.n_lights != 1 || L.lights.size() != 1 || (L.lights[0].type != 0 && L.lights[0].type != 1) || w.d.n_instances != 0 || w.d.n_objects != 0 ||
        !L.spheres.empty() || L.wide.empty() || L.nPrims == 0 || L.nPrims >= (1u << 28))
        return HPRT_OK;
    const bool distant = L.lights[0].type == 1;
    if (distant && !(L.worldRadius > 0.f)) return HPRT_OK;
    for (uint32_t i = 0; i < L.nPrims; ++i) if ((f2u(L.tris[3 * (size_t)i].w) & TAG_KIND_MASK) != 0u) return HPRT_OK;
    static_assert(sizeof(float4) == 16, "triangle records are read as 12 floats per primitive");
    // at most 1 GiB of device image (HPRT_SHADOW_GRID_MAX_MB; the kernel forms 32-bit byte offsets into it): a finer grid is halved
    // until its image fits
    const size_t capMb = [] { const char *e = getenv("HPRT_SHADOW_GRID_MAX_MB"); return e ? (size_t)std::max(1l, atol(e)) : (size_t)1024; }();
    const size_t capBytes = std::min(capMb << 20, (size_t)0xffff0000u);
    const size_t faces = distant ? 1 : 6;
    L.gridKind = distant ? GridKind::Distant : GridKind::Point;
    ShadowGrid &lists = L.grid.lists;
    for (uint32_t R = distant ? DistantGridResFromEnv() : ShadowGridResFromEnv();; R = std::max(1u, lists.R / 2)) {
        while (R > 1 && faces * R * R * SG_BLOCK_WORDS * sizeof(uint32_t) > capBytes) R /= 2;      // (the blocks alone)
        // no image that fits holds more entries: the records, and two in every block
        const size_t maxEntries = capBytes / (SG_RECORD_WORDS * sizeof(uint32_t)) + (size_t)SG_BLOCK_SLOTS * faces * R * R;
        if (distant) BuildDistantGrid(&L.tris[0].x, L.primSingle.data(), L.nPrims, L.lights[0].pos, L.wbMin, L.wbMax, R, maxEntries, mode < 0 ? SG_MAX_CANDIDATES : 0.0, &L.grid);
        else BuildShadowGrid(&L.tris[0].x, L.primSingle.data(), L.nPrims, L.lights[0].pos, L.wbMin, L.wbMax, R, maxEntries, mode < 0 ? SG_MAX_CANDIDATES : 0.0, &lists);
        if (!lists.eligible) return HPRT_OK;
        if (ShadowGridImageBytes(lists) <= capBytes) break;
        if (lists.R == 1) { L.gridKind = GridKind::None; L.grid = DistantGrid(); return HPRT_OK; }      // (not even one cell per face fits: the scene keeps the walk)
    }
    PackShadowGrid(lists, &L.tris[0].x, &L.gridImage);
    return HPRT_OK;
}

// Object instances, and the instance primitives of the top level with their transforms moved next to them (dev_scene.h,
// TAG_INST_INLINE / topEntry)
int LayoutInstances(Work &w) {
    const HprtSceneDesc *d = &w.d;
    SceneLayout &L = w.L;
    L.instances.resize(d->n_instances);
    for (uint32_t i = 0; i < d->n_instances; ++i) {
        const HprtInstanceDesc &in = d->instances[i];
        DevInstance &o = L.instances[i];
        memcpy(o.i2w.m, in.instance_to_world, 64); memcpy(o.w2i.m, in.world_to_instance, 64);
        const size_t ai = 1 + (size_t)in.object;
        // more than one primitive: the object's aggregate; one: that primitive itself, without a bounds test (core/api.cpp:1798-1806)
        o.root = w.aggs[ai].nPrims > 1 ? (int32_t)w.pairBase[ai] : ~(int32_t)w.primBase[ai];
        bool ident = true;                                   // Transform::IsIdentity, core/transform.h:148-155
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) if (o.i2w.m[r][c] != (r == c ? 1.f : 0.f)) ident = false;
        o.identity = ident ? 1u : 0u; o.pad[0] = o.pad[1] = 0u;
        // the entry into the wide records (k_walk4): the object's own tree, or its one primitive as a leaf "already reached" (no bounds test)
        if (!L.wide.empty()) o.pad[0] = w.aggs[ai].nPrims > 1 ? (uint32_t)w.wideBase[ai] : ((~(uint32_t)w.primBase[ai]) & ~WIDE_LEAF_FIRST);
    }
    if (!d->n_instances) return HPRT_OK;
    const uint32_t nTop = w.aggs[0].nPrims;
    L.topEntry.assign(nTop, make_float4(0.f, 0.f, 0.f, 0.f));
    if (!L.wide.empty()) L.topEntryWide.assign(nTop, make_float4(0.f, 0.f, 0.f, 0.f));
    for (uint32_t oi = 0; oi < nTop; ++oi) {
        float4 *r = &L.tris[3 * ((size_t)w.primBase[0] + oi)];
        const uint32_t tag = f2u(r[0].w);
        if ((tag & TAG_KIND_MASK) != TAG_INSTANCE) continue;
        const DevInstance &in = L.instances[f2u(r[2].w)];
        const float (*m)[4] = in.w2i.m;
        if (!(m[3][0] == 0.f && m[3][1] == 0.f && m[3][2] == 0.f && m[3][3] == 1.f)) continue;      // projective: the kernel reads DevInstance
        r[0] = make_float4(m[0][0], m[0][1], m[0][2], u2f(tag | TAG_INST_INLINE));
        r[1] = make_float4(m[1][0], m[1][1], m[1][2], r[1].w);
        r[2] = make_float4(m[2][0], m[2][1], m[2][2], r[2].w);
        L.topEntry[oi] = make_float4(m[0][3], m[1][3], m[2][3], u2f((uint32_t)in.root));
        if (!L.wide.empty()) L.topEntryWide[oi] = make_float4(m[0][3], m[1][3], m[2][3], u2f(in.pad[0]));
    }
    return HPRT_OK;
}

}  // namespace

int BuildSceneLayout(const HprtSceneDesc &d, SceneLayout *out) {
    Work w{d, *out};
    // HPRT_INLINE_MATERIAL_MAX can only lower the limit: the tests reach the shapes[] lookup of larger indices with it
    w.inlineMaterialMax = TAG_MATERIAL_MAX;
    if (const char *e = getenv("HPRT_INLINE_MATERIAL_MAX")) { const long v = atol(e); w.inlineMaterialMax = v < 0 ? 0u : (uint32_t)std::min<long>(v, (long)TAG_MATERIAL_MAX); }
    // validation first (nothing below reads past what it has checked), then the layout in dependency order
    for (int (*stage)(Work &) : {ValidateArrays, ValidateShapes, GatherAggregates, CheckAggregates, ValidateLights}) if (int rc = stage(w)) return rc;
    out->nPrims = w.primBase.back();
    out->topOrder.assign(d.prim_order, d.prim_order + d.n_prims);
    out->instanced = d.n_instances != 0;
    for (uint32_t k = 0; k < d.n_objects; ++k) {
        out->objectOrder.emplace_back(d.objects[k].prim_order, d.objects[k].prim_order + d.objects[k].n_prims);
        out->objectPrimBase.push_back(w.primBase[1 + (size_t)k]);
    }
    for (uint32_t i = 0; i < d.n_instances; ++i) out->instanceObject.push_back(d.instances[i].object);
    for (int (*stage)(Work &) : {LayoutShapes, LayoutPrimitives, LayoutMaterials, LayoutTextures, LayoutLights, LayoutEnvLights,
                                 LayoutLightDistribution, LayoutPairs, LayoutWide, LayoutInstances, LayoutShadowGrid})
        if (int rc = stage(w)) return rc;
    return HPRT_OK;
}

int LayoutTagsForDebug(const HprtSceneDesc &d, std::vector<uint32_t> *tags, std::vector<uint32_t> *primShape, std::vector<uint32_t> *shapeFlags,
                       std::vector<int32_t> *shapeMaterial) {
    SceneLayout L;
    if (int rc = BuildSceneLayout(d, &L)) return rc;
    for (uint32_t i = 0; i < L.nPrims; ++i) { tags->push_back(f2u(L.tris[3 * (size_t)i].w)); primShape->push_back(f2u(L.tris[3 * (size_t)i + 1].w)); }
    for (const DevShape &s : L.shapes) { shapeFlags->push_back(s.flags); shapeMaterial->push_back(s.material); }
    return HPRT_OK;
}

// RadicalInverse(0..4, i), i < 128 (core/lowdiscrepancy.cpp:2478-2488, 389-403): the 3D point and the 2D light sample of
// SpatialLightDistribution::ComputeDistribution's 128 samples per voxel, as [5][128]
void VoxelSamplePoints(float *out) {
    const int bases[5] = {2, 3, 5, 7, 11};
    for (int b = 0; b < 5; ++b)
        for (uint32_t i = 0; i < 128; ++i) {
            float v;
            if (b == 0) {
                uint32_t n = i;      // ReverseBits32(a) * 0x1p-32, evaluated in double
                n = (n << 16) | (n >> 16); n = ((n & 0x00ff00ffu) << 8) | ((n & 0xff00ff00u) >> 8); n = ((n & 0x0f0f0f0fu) << 4) | ((n & 0xf0f0f0f0u) >> 4);
                n = ((n & 0x33333333u) << 2) | ((n & 0xccccccccu) >> 2); n = ((n & 0x55555555u) << 1) | ((n & 0xaaaaaaaau) >> 1);
                v = (float)((double)n * 0x1p-32);
            } else {
                const int base = bases[b];
                const float invBase = (float)1 / (float)base;
                uint64_t reversedDigits = 0, a = i;
                float invBaseN = 1;
                while (a) { uint64_t next = a / base, digit = a - next * base; reversedDigits = reversedDigits * base + digit; invBaseN *= invBase; a = next; }
                v = sel_min((float)reversedDigits * invBaseN, HPRT_ONE_MINUS_EPS);
            }
            out[128 * b + i] = v;
        }
}

}  // namespace hprt

// Diagnostics hook (not part of include/hprt.h): the 128 sample points of a voxel, RadicalInverse(0..4, i) as [5][128]
extern "C" __attribute__((visibility("default"))) int hprt_debug_voxel_points(float out[640]) { if (!out) return HPRT_E_INVALID; hprt::VoxelSamplePoints(out); return HPRT_OK; }

namespace hprt {
int LayoutGridsForDebug(const HprtSceneDesc &d, double out8[8]) {
    SceneLayout L;
    if (int rc = BuildSceneLayout(d, &L)) return rc;
    const ShadowGrid &g = L.grid.lists;
    const bool point = L.gridKind == GridKind::Point, distant = L.gridKind == GridKind::Distant;
    for (int i = 0; i < 8; ++i) out8[i] = 0.0;
    if (point) { out8[0] = g.eligible ? 1 : 0; out8[1] = g.R; }
    if (distant) {
        out8[2] = g.eligible ? 1 : 0; out8[3] = g.R; out8[4] = (double)g.entries.size(); out8[5] = g.nNear;
        out8[6] = g.eligible ? (double)L.gridImage.bytes() : 0.0; out8[7] = g.longest;
    }
    return HPRT_OK;
}
}  // namespace hprt
