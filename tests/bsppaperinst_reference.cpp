// Test-side restatement of an instanced Accelerator "bsppaper" / "bsppaperkd" scene of the fork: BSP::Intersect / IntersectP
// (accelerators/BSP.cpp:27-165) — kd-aware: BSPKd::Intersect / IntersectP (accelerators/BSPKd.cpp:25-171) — over the top-level
// tree, TransformedPrimitive::Intersect / IntersectP (core/primitive.cpp:77-102) at every leaf primitive that is an object
// instance, and the same walk again over the tree pbrtObjectInstance (core/api.cpp:1794-1819) builds for an object of more than one
// primitive (an object of one primitive is wrapped as it is, :1798).  Written independently of thesis-pbrt-v3_amd/csrc/ over the
// oracle's scene loader, primitive tests and ray transform (oracle/, included read-only) and tests/tree_reference.h's root
// interval.  The interior steps and the builds are those of tests/bsppaper_reference.cpp and tests/bsppaperkd_reference.cpp, the
// restatements the library's builder and single-level walks are already held to.  tests/bsppaperkd_reference.cpp includes
// tests/bsppaper_reference.cpp whole, so ONE include in ONE namespace brings both (a second would define the extern "C" entry
// points of the general BSP tree twice); their Build / BuildKd are fed THIS file's primitive lists — an object's primitives in
// object space, the top level's with an instance as a non-triangle bounded by TransformedPrimitive::WorldBound, which therefore
// has no planes of its own (Planes() of a non-triangle is empty) and projects its bound's corners (GetBounds).  Both node types
// are the same 20 bytes, so the trees are held as BSPKdNode arrays and a plain node is handed to BspStep as a BSPNode copy.  The
// trees the walk takes are GIVEN: the arrays copied out of the library's handle, or made by hand.  Compiled with g++ at test time
// (tests/bsppaperinst_ref.py), driven through ctypes.  It pins nothing against a reference binary: the device walk is held to
// THIS walk ("parity unpinned").
#include "tree_reference.h"

namespace ref {
#include "bsppaperkd_reference.cpp"
}

namespace {

typedef ref::BSPKdNode Node20;       // BSPNode and BSPKdNode: the same 20 bytes, read through the handle's flag layout
static_assert(sizeof(ref::BSPNode) == sizeof(Node20), "one node size");
typedef TreeT<Node20> RTree;
const ref::Tree kNoTree;            // BspStep reads nothing of its tree

// per ray: nodes (nbNodeTraversals), interior nodes (bspTreeNodeTraversals, kd-aware: kdTreeNodeTraversals + bspTreeNodeTraversals),
// leaves, the kd share (kd interior nodes of a kd-aware tree) — summed over both levels as r.stats += ray.stats
// (core/primitive.cpp:84,100) sums them — and the most todo entries the ray held at once, counting the device walk's one list: the
// top level's entries, one saved position while inside an instance, the object's entries
struct Walk2 { uint64_t nodes = 0, interior = 0, leaves = 0, kd = 0; uint32_t maxTodo = 0; };

struct InstScene {
    Scene scene;
    std::vector<BVH> objectBvh;      // for the ordered numbering of every aggregate and the primitive tests
    BVH bvh;
    std::vector<uint32_t> toOrdered;                 // top level: creation number -> ordered position
    std::vector<std::vector<uint32_t>> objToOrdered;  // per object
    bool kdAware = false;
    ref::BspKdStep kdStep;           // kdStep.dotOnly: the control, the dot-product step at every node
    RTree top;
    std::vector<RTree> objects;      // no nodes: an object of one primitive

    struct ToDo { const Node20 *node; Float tMin, tMax; };

    static ref::BSPNode Plain(const Node20 *n) { ref::BSPNode b; memcpy(&b, n, sizeof(b)); return b; }
    uint32_t Shift() const { return kdAware ? ref::BspKdStep::Shift(RTree()) : ref::BspStep::Shift(kNoTree); }
    bool IsLeaf(const RTree &t, const Node20 *n) const {
        if (kdAware) return ref::BspKdStep::IsLeaf(t, n);
        const ref::BSPNode b = Plain(n);
        return ref::BspStep::IsLeaf(kNoTree, &b);
    }
    bool Kd(const RTree &t, const Node20 *n) const { return kdAware && ref::BspKdStep::Kd(t, n); }
    void Interior(const RTree &t, const Node20 *n, const Ray &ray, const V3 &invDir, Float *tPlane, bool *belowFirst) const {
        if (kdAware) { kdStep.Interior(t, n, ray, invDir, tPlane, belowFirst); return; }
        const ref::BSPNode b = Plain(n);
        ref::BspStep::Interior(kNoTree, &b, ray, invDir, tPlane, belowFirst);
    }

    // BSP::Intersect / BSPKd::Intersect over one tree; `held`: the entries the device's one list holds below this level's
    template <class PrimFn> bool WalkClosest(const RTree &tree, const Ray &ray, uint32_t held, Walk2 &wc, PrimFn prim) const {
        const uint32_t off = Shift();
        Float tMin, tMax;
        if (!RootInterval(tree.bounds, ray, &tMin, &tMax)) return false;
        const V3 invDir(1 / ray.d.x, 1 / ray.d.y, 1 / ray.d.z);
        ToDo todo[64];
        uint32_t todoPos = 0;
        bool hit = false;
        const Node20 *node = &tree.nodes[0];
        while (node != nullptr) {
            if (ray.tMax < tMin) break;
            ++wc.nodes;
            if (!IsLeaf(tree, node)) {
                ++wc.interior;
                if (Kd(tree, node)) ++wc.kd;
                Float tPlane; bool belowFirst;
                Interior(tree, node, ray, invDir, &tPlane, &belowFirst);
                const Node20 *first, *second;
                if (belowFirst) { first = node + 1; second = &tree.nodes[node->aboveChild >> off]; }
                else { first = &tree.nodes[node->aboveChild >> off]; second = node + 1; }
                if (tPlane > tMax || tPlane <= 0) node = first;
                else if (tPlane < tMin) node = second;
                else {
                    todo[todoPos].node = second; todo[todoPos].tMin = tPlane; todo[todoPos].tMax = tMax; ++todoPos;
                    wc.maxTodo = std::max(wc.maxTodo, held + todoPos);
                    node = first; tMax = tPlane;
                }
            } else {
                ++wc.leaves;
                const uint32_t np = node->nPrims >> off;
                for (uint32_t i = 0; i < np; ++i) {
                    const uint32_t p = np == 1 ? node->onePrimitive : tree.primitiveIndices[node->primitiveIndicesOffset + i];
                    if (prim(p, held + todoPos)) hit = true;
                }
                if (todoPos > 0) { --todoPos; node = todo[todoPos].node; tMin = todo[todoPos].tMin; tMax = todo[todoPos].tMax; }
                else break;
            }
        }
        return hit;
    }
    // BSP::IntersectP / BSPKd::IntersectP: the leaf test comes first, no early-out on tMin
    template <class PrimFn> bool WalkAny(const RTree &tree, const Ray &ray, uint32_t held, Walk2 &wc, PrimFn prim) const {
        const uint32_t off = Shift();
        Float tMin, tMax;
        if (!RootInterval(tree.bounds, ray, &tMin, &tMax)) return false;
        const V3 invDir(1 / ray.d.x, 1 / ray.d.y, 1 / ray.d.z);
        ToDo todo[64];
        uint32_t todoPos = 0;
        const Node20 *node = &tree.nodes[0];
        while (node != nullptr) {
            ++wc.nodes;
            if (IsLeaf(tree, node)) {
                ++wc.leaves;
                const uint32_t np = node->nPrims >> off;
                for (uint32_t i = 0; i < np; ++i) {
                    const uint32_t p = np == 1 ? node->onePrimitive : tree.primitiveIndices[node->primitiveIndicesOffset + i];
                    if (prim(p, held + todoPos)) return true;
                }
                if (todoPos > 0) { --todoPos; node = todo[todoPos].node; tMin = todo[todoPos].tMin; tMax = todo[todoPos].tMax; }
                else break;
            } else {
                ++wc.interior;
                if (Kd(tree, node)) ++wc.kd;
                Float tPlane; bool belowFirst;
                Interior(tree, node, ray, invDir, &tPlane, &belowFirst);
                const Node20 *first, *second;
                if (belowFirst) { first = node + 1; second = &tree.nodes[node->aboveChild >> off]; }
                else { first = &tree.nodes[node->aboveChild >> off]; second = node + 1; }
                if (tPlane > tMax || tPlane <= 0) node = first;
                else if (tPlane < tMin) node = second;
                else {
                    todo[todoPos].node = second; todo[todoPos].tMin = tPlane; todo[todoPos].tMax = tMax; ++todoPos;
                    wc.maxTodo = std::max(wc.maxTodo, held + todoPos);
                    node = first; tMax = tPlane;
                }
            }
        }
        return false;
    }

    // TransformedPrimitive::Intersect (core/primitive.cpp:77-93); the interaction's transform back to world space is the shading
    // side's business (the hit record carries t, primitive, instance and barycentrics)
    bool InstanceIntersect(int instIndex, const Ray &r, uint32_t held, SurfaceInteraction *isect, Counters &ctr, Walk2 &wc) const {
        const Instance &in = scene.instances[instIndex];
        Ray ray = XfRay(in.w2i, r);
        const BVH &ob = objectBvh[in.object];
        const RTree &tree = objects[in.object];
        wc.maxTodo = std::max(wc.maxTodo, held + 1);      // the device walk's saved top-level position
        bool hit;
        if (ob.plist->size() > 1) {
            const std::vector<uint32_t> &map = objToOrdered[in.object];
            hit = WalkClosest(tree, ray, held + 1, wc, [&](uint32_t p, uint32_t) { return ob.PrimIntersect(map[p], ray, isect, ctr); });
        } else hit = ob.PrimIntersect(0, ray, isect, ctr);
        if (!hit) return false;
        r.tMax = ray.tMax;
        isect->inst = instIndex;
        return true;
    }
    bool InstanceIntersectP(int instIndex, const Ray &r, uint32_t held, Counters &ctr, Walk2 &wc) const {
        const Instance &in = scene.instances[instIndex];
        Ray ray = XfRay(in.w2i, r);
        const BVH &ob = objectBvh[in.object];
        wc.maxTodo = std::max(wc.maxTodo, held + 1);
        if (ob.plist->size() > 1) {
            const std::vector<uint32_t> &map = objToOrdered[in.object];
            return WalkAny(objects[in.object], ray, held + 1, wc, [&](uint32_t p, uint32_t) { return ob.PrimIntersectP(map[p], ray, ctr); });
        }
        return ob.PrimIntersectP(0, ray, ctr);
    }

    bool Intersect(const Ray &ray, SurfaceInteraction *isect, Counters &ctr, Walk2 &wc) const {
        return WalkClosest(top, ray, 0, wc, [&](uint32_t p, uint32_t held) {
            const PrimRef &pr = scene.prims[p];
            if (pr.shape < 0) return InstanceIntersect(pr.local, ray, held, isect, ctr, wc);
            return bvh.PrimIntersect(toOrdered[p], ray, isect, ctr);
        });
    }
    bool IntersectP(const Ray &ray, Counters &ctr, Walk2 &wc) const {
        return WalkAny(top, ray, 0, wc, [&](uint32_t p, uint32_t held) {
            const PrimRef &pr = scene.prims[p];
            if (pr.shape < 0) return InstanceIntersectP(pr.local, ray, held, ctr, wc);
            return bvh.PrimIntersectP(toOrdered[p], ray, ctr);
        });
    }

    // The primitive list a tree is built over, in creation order (object < 0: the top level): a triangle with its three vertices
    // (an object's in object space), anything else — a sphere, an instance — as its bound alone; an instance's is
    // TransformedPrimitive::WorldBound with the oracle's transform (BVH::PrimWorldBound)
    std::vector<Prim> Prims(int object) const {
        const BVH &b = object < 0 ? bvh : objectBvh[object];
        const std::vector<PrimRef> &list = object < 0 ? scene.prims : scene.objectPrims[object];
        std::vector<Prim> out(list.size());
        for (size_t i = 0; i < out.size(); ++i) {
            const PrimRef &pr = list[i];
            out[i].wb = b.PrimWorldBound((uint32_t)i);
            out[i].tri = false;
            if (pr.shape < 0) continue;
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

B3 UnionOf(const BVH &b, size_t n) {
    B3 u;
    for (size_t i = 0; i < n; ++i) u = Union(u, b.PrimWorldBound((uint32_t)i));
    return u;
}

}  // namespace

extern "C" {

const char *bspinstref_last_error() { return g_err.c_str(); }

// a baked scene WITH instances and the oracle's BVHs over it (the ordered numbering of every aggregate: top level first, then each
// object's); the trees come through bspinstref_set_tree; kdAware: BSPKdNode's flags and interior step.  Every tree's bounds start
// as GenericBSP::bounds: the union of its primitives' bounds.
void *bspinstref_scene_load(const char *path, int kdAware) {
    InstScene *r = new InstScene();
    std::string err;
    if (!LoadScene(path, &r->scene, &err)) { g_err = err; delete r; return nullptr; }
    if (r->scene.instances.empty()) { g_err = "scene without instances"; delete r; return nullptr; }
    r->kdAware = kdAware != 0;
    const size_t nObj = r->scene.objectPrims.size();
    r->objectBvh.resize(nObj);
    uint32_t base = (uint32_t)r->scene.prims.size();
    for (size_t o = 0; o < nObj; ++o) {
        r->objectBvh[o].Build(&r->scene, &r->scene.objectPrims[o], &r->objectBvh, base);
        base += (uint32_t)r->scene.objectPrims[o].size();
    }
    r->bvh.Build(&r->scene, &r->scene.prims, &r->objectBvh, 0);
    auto invert = [](const std::vector<uint32_t> &order) {
        std::vector<uint32_t> inv(order.size());
        for (size_t i = 0; i < order.size(); ++i) inv[order[i]] = (uint32_t)i;
        return inv;
    };
    r->toOrdered = invert(r->bvh.primOrder);
    r->objects.resize(nObj); r->objToOrdered.resize(nObj);
    for (size_t o = 0; o < nObj; ++o) {
        r->objToOrdered[o] = invert(r->objectBvh[o].primOrder);
        r->objects[o].bounds = UnionOf(r->objectBvh[o], r->scene.objectPrims[o].size());
    }
    r->top.bounds = UnionOf(r->bvh, r->scene.prims.size());
    return r;
}
void bspinstref_scene_free(void *h) { delete (InstScene *)h; }
// out[0..2] = top-level primitives, object definitions, instances
void bspinstref_counts(void *h, uint32_t out[3]) {
    const InstScene *r = (const InstScene *)h;
    out[0] = (uint32_t)r->scene.prims.size(); out[1] = (uint32_t)r->scene.objectPrims.size(); out[2] = (uint32_t)r->scene.instances.size();
}
// object < 0: the top level.  Returns the primitive count; with the arrays given, the list the tree is built over in creation
// order: the triangle flag, the three vertices (zeros for a non-triangle) and the bound
size_t bspinstref_prims(void *h, int object, uint8_t *isTri, float *p9, float *bmin, float *bmax) {
    const InstScene *r = (const InstScene *)h;
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
void bspinstref_tree_bounds(void *h, int object, float out6[6]) {
    const InstScene *r = (const InstScene *)h;
    const B3 &b = object < 0 ? r->top.bounds : r->objects[object].bounds;
    for (int k = 0; k < 3; ++k) { out6[k] = b.pMin[k]; out6[3 + k] = b.pMax[k]; }
}
// The test-side Build (tests/bsppaper_reference.cpp, kd-aware BuildKd of tests/bsppaperkd_reference.cpp) over the primitive list of
// the top level (object < 0) or of one object; sizes[0..1] = nodes, primitiveIndices entries.
void *bspinstref_build(void *h, int object, int isectCost, int travCost, int kdTravCost, float emptyBonus, int maxPrims, int maxDepth, uint32_t sizes[2]) {
    const InstScene *r = (const InstScene *)h;
    const std::vector<Prim> prims = r->Prims(object);
    RTree *t = new RTree();
    if (r->kdAware) ref::BuildKd(prims, (uint32_t)isectCost, (uint32_t)travCost, (uint32_t)kdTravCost, emptyBonus, (uint32_t)maxPrims, (uint32_t)maxDepth, t);
    else {
        ref::Tree p;
        ref::Build(prims, (uint32_t)isectCost, (uint32_t)travCost, emptyBonus, (uint32_t)maxPrims, (uint32_t)maxDepth, &p);
        t->nodes.resize(p.nodes.size());
        if (!p.nodes.empty()) memcpy(static_cast<void *>(t->nodes.data()), p.nodes.data(), p.nodes.size() * sizeof(Node20));
        t->primitiveIndices = p.primitiveIndices; t->bounds = p.bounds;
    }
    sizes[0] = (uint32_t)t->nodes.size(); sizes[1] = (uint32_t)t->primitiveIndices.size();
    return t;
}
void bspinstref_built_copy(void *tree, void *nodes20, uint32_t *idx, float *bounds6) {
    const RTree *t = (const RTree *)tree;
    CopyTree(*t, nodes20, idx, nullptr);
    if (bounds6) for (int k = 0; k < 3; ++k) { bounds6[k] = t->bounds.pMin[k]; bounds6[3 + k] = t->bounds.pMax[k]; }
}
void bspinstref_built_free(void *tree) { delete (RTree *)tree; }
// the arrays as hprt_bsppaperinst_copy / hprt_bsppaperinst_object_copy write them, 5 words per node (or made by hand); bounds6 (may be null): the tree's
// bounds where they are not the union of its primitives'
void bspinstref_set_tree(void *h, int object, size_t nNodes, const void *nodes20, size_t nIdx, const uint32_t *idx, const float *bounds6) {
    InstScene *r = (InstScene *)h;
    RTree &t = object < 0 ? r->top : r->objects[object];
    t.nodes.resize(nNodes);
    if (nNodes) memcpy(static_cast<void *>(t.nodes.data()), nodes20, nNodes * sizeof(Node20));
    t.primitiveIndices.assign(idx, idx + nIdx);
    if (bounds6) { t.bounds.pMin = V3(bounds6[0], bounds6[1], bounds6[2]); t.bounds.pMax = V3(bounds6[3], bounds6[4], bounds6[5]); }
}
// dot != 0: a kd-aware scene walks every interior node with the dot-product step (the control of tests/bsppaperkd_reference.cpp)
void bspinstref_dot_only(void *h, int dot) { ((InstScene *)h)->kdStep.dotOnly = dot != 0; }
// counters per ray, 6 columns: nodes, interior nodes, leaves, triangle tests, sphere tests, kd interior nodes; prim: the ordered
// primitive over all aggregates; inst: the instance the hit went through or -1; maxTodo (may be null): the entries the one list
// held at most
void bspinstref_intersect(void *h, size_t n, const float *o, const float *d, const float *tmax, float *tOut, int32_t *primOut, int32_t *instOut,
                           float *bary, uint64_t *counters6, uint32_t *maxTodo) {
    const InstScene *r = (const InstScene *)h;
    for (size_t i = 0; i < n; ++i) {
        Ray ray(V3(o[3 * i], o[3 * i + 1], o[3 * i + 2]), V3(d[3 * i], d[3 * i + 1], d[3 * i + 2]), tmax[i]);
        SurfaceInteraction si; Counters c; Walk2 wc;
        const bool hit = r->Intersect(ray, &si, c, wc);
        tOut[i] = ray.tMax; primOut[i] = hit ? si.ordered : -1; instOut[i] = hit ? si.inst : -1;
        bary[3 * i] = hit ? si.b0 : 0.f; bary[3 * i + 1] = hit ? si.b1 : 0.f; bary[3 * i + 2] = hit ? si.b2 : 0.f;
        uint64_t *c6 = &counters6[6 * i];
        c6[0] = wc.nodes; c6[1] = wc.interior; c6[2] = wc.leaves; c6[3] = c.triTests; c6[4] = c.sphereTests; c6[5] = wc.kd;
        if (maxTodo) maxTodo[i] = wc.maxTodo;
    }
}
void bspinstref_occluded(void *h, size_t n, const float *o, const float *d, const float *tmax, uint8_t *occ, uint64_t *counters6, uint32_t *maxTodo) {
    const InstScene *r = (const InstScene *)h;
    for (size_t i = 0; i < n; ++i) {
        Ray ray(V3(o[3 * i], o[3 * i + 1], o[3 * i + 2]), V3(d[3 * i], d[3 * i + 1], d[3 * i + 2]), tmax[i]);
        Counters c; Walk2 wc;
        occ[i] = r->IntersectP(ray, c, wc) ? 1 : 0;
        uint64_t *c6 = &counters6[6 * i];
        c6[0] = wc.nodes; c6[1] = wc.interior; c6[2] = wc.leaves; c6[3] = c.triTestsP; c6[4] = c.sphereTestsP; c6[5] = wc.kd;
        if (maxTodo) maxTodo[i] = wc.maxTodo;
    }
}

}  // extern "C"
