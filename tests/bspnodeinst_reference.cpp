// Test-side restatement of the BUILD of an instanced scene under one of the fork's nine node-based accelerators ("bsparbitrary",
// "bspcluster", "bsprandom", each plain, withkd or fastkd): pbrtObjectInstance (core/api.cpp:1794-1819) hands MakeAccelerator the
// primitives of every object that has more than one, in object space, and pbrtWorldEnd hands it the top-level list, in which an
// instance is a TransformedPrimitive (core/primitive.h:144-182) — Normal() (0, 0, 0), getBounds Primitive's over the 8 corners of
// its WorldBound.  Written independently of thesis-pbrt-v3_amd/csrc/ over the oracle's scene loader and bounds (oracle/, included
// read-only); the builds are BuildNodeBased / BuildFastKd of tests/bspnode_reference.cpp, the restatements the library's
// single-level builder is already held to, included whole (its bspnoderef_* entry points come along unused) and fed THIS file's
// primitive lists: a triangle with its three vertices, anything else — a sphere, an instance — as its bound alone, which is all
// Normal() and GetBounds() read of a non-triangle.  Every tree starts its own std::mt19937(seed), as the library's does (the
// reference seeds from std::random_device: "parity unpinned").  The two-level WALK over such trees is
// tests/bsppaperinst_reference.cpp's, which takes any trees of this node layout (BspPaperInstScene.take).  Compiled with g++ at
// test time (tests/bspnodeinst_ref.py), driven through ctypes.
#include "bspnode_reference.cpp"

namespace {

struct NodeInstScene {
    Scene scene;
    std::vector<BVH> objectBvh;      // for PrimWorldBound: an instance's bound needs its object's
    BVH bvh;

    // The primitive list a tree is built over, in creation order (object < 0: the top level)
    std::vector<Prim> Prims(int object) const {
        const BVH &b = object < 0 ? bvh : objectBvh[object];
        const std::vector<PrimRef> &list = object < 0 ? scene.prims : scene.objectPrims[object];
        std::vector<Prim> out(list.size());
        for (size_t i = 0; i < out.size(); ++i) {
            const PrimRef &pr = list[i];
            out[i].wb = b.PrimWorldBound((uint32_t)i);      // an instance's: TransformedPrimitive::WorldBound
            out[i].tri = false;
            if (pr.shape < 0) continue;                     // an instance: no normal, no vertices
            const ShapeRec &sh = scene.shapes[pr.shape];
            out[i].tri = sh.kind == SHAPE_MESH;
            if (out[i].tri) {
                const Mesh &m = scene.meshes[sh.meshIndex];
                for (int k = 0; k < 3; ++k) out[i].p[k] = m.p[m.idx[3 * pr.local + k]];
            }
        }
        return out;
    }
};

}  // namespace

extern "C" {

const char *bspnodeinstref_last_error() { return g_err.c_str(); }

void *bspnodeinstref_scene_load(const char *path) {
    NodeInstScene *r = new NodeInstScene();
    std::string err;
    if (!LoadScene(path, &r->scene, &err)) { g_err = err; delete r; return nullptr; }
    if (r->scene.instances.empty()) { g_err = "scene without instances"; delete r; return nullptr; }
    const size_t nObj = r->scene.objectPrims.size();
    r->objectBvh.resize(nObj);
    uint32_t base = (uint32_t)r->scene.prims.size();
    for (size_t o = 0; o < nObj; ++o) {
        r->objectBvh[o].Build(&r->scene, &r->scene.objectPrims[o], &r->objectBvh, base);
        base += (uint32_t)r->scene.objectPrims[o].size();
    }
    r->bvh.Build(&r->scene, &r->scene.prims, &r->objectBvh, 0);
    return r;
}
void bspnodeinstref_scene_free(void *h) { delete (NodeInstScene *)h; }
// out[0..2] = top-level primitives, object definitions, instances
void bspnodeinstref_counts(void *h, uint32_t out[3]) {
    const NodeInstScene *r = (const NodeInstScene *)h;
    out[0] = (uint32_t)r->scene.prims.size(); out[1] = (uint32_t)r->scene.objectPrims.size(); out[2] = (uint32_t)r->scene.instances.size();
}
// object < 0: the top level.  Returns the primitive count; with the arrays given, the list the tree is built over in creation
// order: the triangle flag, the three vertices (zeros for a non-triangle) and the bound
size_t bspnodeinstref_prims(void *h, int object, uint8_t *isTri, float *p9, float *bmin, float *bmax) {
    const NodeInstScene *r = (const NodeInstScene *)h;
    const std::vector<Prim> prims = r->Prims(object);
    if (isTri && p9 && bmin && bmax)
        for (size_t i = 0; i < prims.size(); ++i) {
            const Prim &p = prims[i];
            isTri[i] = p.tri ? 1 : 0;
            for (int v = 0; v < 3; ++v) for (int k = 0; k < 3; ++k) p9[9 * i + 3 * v + k] = p.tri ? p.p[v][k] : 0.f;
            for (int k = 0; k < 3; ++k) { bmin[3 * i + k] = p.wb.pMin[k]; bmax[3 * i + k] = p.wb.pMax[k]; }
        }
    return prims.size();
}
// BuildNodeBased / BuildFastKd (tests/bspnode_reference.cpp) over the primitive list of the top level (object < 0) or of one
// object, from a fresh engine; sizes[0..1] = nodes, primitiveIndices entries; null (last_error) where the reference's build is
// undefined
void *bspnodeinstref_build(void *h, int object, int chooser, int form, int K, uint32_t seed, int isectCost, int travCost, int kdTravCost, float emptyBonus,
                           int maxPrims, int maxDepth, uint32_t sizes[2]) {
    const NodeInstScene *r = (const NodeInstScene *)h;
    BuiltTree *t = new BuiltTree();
    t->form = form;
    if (!BuildForm(r->Prims(object), chooser, form, (uint32_t)K, seed, (uint32_t)isectCost, (uint32_t)travCost, (uint32_t)kdTravCost, emptyBonus,
                   (uint32_t)maxPrims, (uint32_t)maxDepth, &t->plain, &t->kd)) { delete t; return nullptr; }
    sizes[0] = (uint32_t)(form == FASTKD ? t->kd.nodes.size() : t->plain.nodes.size());
    sizes[1] = (uint32_t)(form == FASTKD ? t->kd.primitiveIndices.size() : t->plain.primitiveIndices.size());
    return t;
}
// nodes20: 5 words per node; bounds6: GenericBSP::bounds, the union of the primitives' bounds
void bspnodeinstref_built_copy(void *tree, void *nodes20, uint32_t *idx, float *bounds6) {
    const BuiltTree *t = (const BuiltTree *)tree;
    if (t->form == FASTKD) CopyTree(t->kd, nodes20, idx, nullptr);
    else CopyTree(t->plain, nodes20, idx, nullptr);
    const B3 &b = t->form == FASTKD ? t->kd.bounds : t->plain.bounds;
    if (bounds6) for (int k = 0; k < 3; ++k) { bounds6[k] = b.pMin[k]; bounds6[3 + k] = b.pMax[k]; }
}
void bspnodeinstref_built_free(void *tree) { delete (BuiltTree *)tree; }

}  // extern "C"
