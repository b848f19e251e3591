// Test-side statement of the stock pbrt-v3 BVH the fork keeps under Accelerator "bvhold" — a top-down build with four ways of
// splitting a range (bucketed surface-area heuristic, spatial middle, median, Morton-ordered treelets joined by a bucketed SAH),
// a depth-first node array and the two stack walks — written from the algorithm's description with this file's own structure
// and names, independently of thesis-pbrt-v3_amd/csrc/, over the oracle's loader, vector type and primitive tests
// (oracle/orc_accel.h, included read-only).  Compiled with g++ at test time (tests/bvhold_ref.py) and driven through ctypes.
// It pins nothing against a reference binary: the library's trees and the device walks are held to THIS ("parity unpinned").
//
// What the description leaves open is settled as the library's header settles it: the top-down build finishes a node's second
// half before its first (what g++ makes of two calls that are arguments of one call), so the second half's leaves are numbered
// first; the Morton build numbers its leaves in sorted order.  The standard algorithms std::partition and std::nth_element are
// part of the algorithm's definition (they decide the order inside a range) and are called as such, over plain pointers.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <deque>
#include <string>
#include <vector>
#include "orc_accel.h"

namespace orc { bool g_use_libm = false; }
using namespace orc;

namespace {

std::string g_err;

enum How { kSah = 0, kMorton = 1, kMiddle = 2, kMedian = 3 };
constexpr int kBins = 12;
constexpr int kMaxStoredLeaf = 65535;

struct Item { uint32_t id; B3 box; V3 mid; };               // a primitive: creation number, world box, box centre
struct Knot { B3 box; Knot *kid[2] = {nullptr, nullptr}; int axis = 0, first = 0, count = 0; };   // count > 0: a leaf
struct Coded { uint32_t code; uint32_t id; };                // a primitive under its 30-bit Morton code
struct Flat { std::vector<LinearBVHNode> nodes; std::vector<uint32_t> sequence; };   // sequence: ordered position -> creation number

int WidestAxis(const B3 &b) {
    const V3 e = b.Diagonal();
    return (e.x > e.y && e.x > e.z) ? 0 : (e.y > e.z ? 1 : 2);
}
// where x sits in [lo, hi] as a fraction; an interval without extent leaves the difference
Float Fraction(Float lo, Float hi, Float x) {
    Float f = x - lo;
    if (hi > lo) f /= hi - lo;
    return f;
}
int BinOf(Float fraction) {
    int b = kBins * fraction;
    return b == kBins ? kBins - 1 : b;
}

struct Bin { int n = 0; B3 box; };
// The cheapest of the 11 cuts between 12 bins: price = fixed + (n_left * area_left + n_right * area_right) / area_whole,
// the first of equal prices.  Both sides are gathered from bin 0 upwards.
int CheapestCut(const Bin *bins, const B3 &whole, Float fixed, Float *priceOut) {
    int best = 0;
    Float bestPrice = 0;
    B3 left;
    int nLeft = 0;
    for (int cut = 0; cut + 1 < kBins; ++cut) {
        left = Union(left, bins[cut].box); nLeft += bins[cut].n;
        B3 right;
        int nRight = 0;
        for (int k = cut + 1; k < kBins; ++k) { right = Union(right, bins[k].box); nRight += bins[k].n; }
        const Float price = fixed + (nLeft * left.SurfaceArea() + nRight * right.SurfaceArea()) / whole.SurfaceArea();
        if (cut == 0 || price < bestPrice) { best = cut; bestPrice = price; }
    }
    *priceOut = bestPrice;
    return best;
}

// ten bits, each moved to every third position; 1024 (a fraction of exactly one) counts as 1023
uint32_t EveryThird(uint32_t v) {
    if (v == 1024u) v = 1023u;
    uint32_t out = 0;
    for (int b = 0; b < 10; ++b) out |= ((v >> b) & 1u) << (3 * b);
    return out;
}

struct Grower {
    int leafCap = 4; How how = kSah;
    std::deque<Knot> pool;
    std::vector<uint32_t> sequence;
    std::string stop;                       // why the reference's build would stop (one of its checks), "" otherwise

    Knot *Fresh() { pool.emplace_back(); return &pool.back(); }
    Knot *Join(int axis, Knot *a, Knot *b) {
        Knot *k = Fresh();
        k->kid[0] = a; k->kid[1] = b; k->axis = axis; k->box = Union(a->box, b->box);
        return k;
    }
    Knot *Leaf(const B3 &box, int first, int count) {
        Knot *k = Fresh();
        k->box = box; k->first = first; k->count = count;
        return k;
    }

    // ---- top-down over [from, to) ----
    Knot *LeafOfRange(const Item *from, const Item *to, const B3 &box) {
        const int first = (int)sequence.size();
        for (const Item *it = from; it != to; ++it) sequence.push_back(it->id);
        return Leaf(box, first, (int)(to - from));
    }
    Knot *TopDown(Item *from, Item *to) {
        const int n = (int)(to - from);
        B3 box, mids;
        for (Item *it = from; it != to; ++it) { box = Union(box, it->box); mids = Union(mids, it->mid); }
        const int axis = WidestAxis(mids);
        const Float lo = mids.pMin[axis], hi = mids.pMax[axis];
        if (n == 1 || lo == hi) return LeafOfRange(from, to, box);
        Item *half = from + n / 2;
        auto byMid = [axis](const Item &a, const Item &b) { return a.mid[axis] < b.mid[axis]; };
        Item *cut = nullptr;
        if (how == kMiddle) {
            const Float centre = (lo + hi) / 2;
            cut = std::partition(from, to, [axis, centre](const Item &it) { return it.mid[axis] < centre; });
            if (cut == from || cut == to) cut = nullptr;             // one-sided: the median decides
        }
        if (how == kSah && n > 2) {
            Bin bins[kBins];
            for (Item *it = from; it != to; ++it) {
                const int b = BinOf(Fraction(lo, hi, it->mid[axis]));
                if (b < 0 || b >= kBins) { if (stop.empty()) stop = "a centre outside the 12 bins"; return LeafOfRange(from, to, box); }
                ++bins[b].n; bins[b].box = Union(bins[b].box, it->box);
            }
            Float price;
            const int at = CheapestCut(bins, box, 1, &price);
            if (!(n > leafCap || price < Float(n))) return LeafOfRange(from, to, box);
            cut = std::partition(from, to, [=](const Item &it) { return BinOf(Fraction(lo, hi, it.mid[axis])) <= at; });
        }
        if (!cut) { std::nth_element(from, half, to, byMid); cut = half; }
        Knot *second = TopDown(cut, to);      // the second half first: see the head of this file
        Knot *first = TopDown(from, cut);
        return Join(axis, first, second);
    }

    // ---- Morton order: treelets of equal top 12 bits, split bit by bit from bit 17 down, joined by a bucketed SAH ----
    const std::vector<Item> *items = nullptr;
    const Coded *sortedBase = nullptr;

    Knot *Linear(const Coded *from, const Coded *to, int bit) {
        const int n = (int)(to - from);
        // bits on which the whole range agrees are passed over; fewer than leafCap primitives, or no bit left, make a leaf
        while (bit >= 0 && n >= leafCap && ((from->code ^ (to - 1)->code) >> bit & 1u) == 0) --bit;
        if (bit < 0 || n < leafCap) {
            B3 box;
            for (const Coded *c = from; c != to; ++c) box = Union(box, (*items)[c->id].box);
            return Leaf(box, (int)(from - sortedBase), n);
        }
        const uint32_t side = from->code >> bit & 1u;
        const Coded *cut = std::partition_point(from, to, [=](const Coded &c) { return (c.code >> bit & 1u) == side; });
        Knot *a = Linear(from, cut, bit - 1);
        Knot *b = Linear(cut, to, bit - 1);
        return Join(bit % 3, a, b);
    }
    Knot *JoinRoots(Knot **from, Knot **to) {
        if (to - from == 1) return *from;
        B3 box, mids;
        for (Knot **k = from; k != to; ++k) { box = Union(box, (*k)->box); mids = Union(mids, ((*k)->box.pMin + (*k)->box.pMax) * 0.5f); }
        const int axis = WidestAxis(mids);
        const Float lo = mids.pMin[axis], hi = mids.pMax[axis];
        if (lo == hi) { if (stop.empty()) stop = "the treelet roots' centres coincide on the widest axis"; return *from; }
        auto binOfRoot = [=](const Knot *k) { return BinOf((((k->box.pMin[axis] + k->box.pMax[axis]) * 0.5f) - lo) / (hi - lo)); };
        Bin bins[kBins];
        for (Knot **k = from; k != to; ++k) {
            const int b = binOfRoot(*k);
            if (b < 0 || b >= kBins) { if (stop.empty()) stop = "a centre outside the 12 bins"; return *from; }
            ++bins[b].n; bins[b].box = Union(bins[b].box, (*k)->box);
        }
        Float price;
        const int at = CheapestCut(bins, box, .125f, &price);
        Knot **cut = std::partition(from, to, [=](const Knot *k) { return binOfRoot(k) <= at; });
        Knot *a = JoinRoots(from, cut);
        Knot *b = JoinRoots(cut, to);
        return Join(axis, a, b);
    }
    Knot *MortonBuild(const std::vector<Item> &all) {
        items = &all;
        B3 mids;
        for (const Item &it : all) mids = Union(mids, it.mid);
        std::vector<Coded> coded(all.size());
        for (size_t i = 0; i < all.size(); ++i) {
            uint32_t cell[3];
            for (int a = 0; a < 3; ++a) cell[a] = (uint32_t)(Fraction(mids.pMin[a], mids.pMax[a], all[i].mid[a]) * 1024);
            coded[i] = Coded{EveryThird(cell[2]) << 2 | EveryThird(cell[1]) << 1 | EveryThird(cell[0]), all[i].id};
        }
        std::stable_sort(coded.begin(), coded.end(), [](const Coded &a, const Coded &b) { return a.code < b.code; });
        sortedBase = coded.data();
        sequence.resize(all.size());
        for (size_t i = 0; i < all.size(); ++i) sequence[i] = coded[i].id;
        std::vector<Knot *> roots;
        for (size_t from = 0; from < coded.size();) {
            size_t to = from + 1;
            while (to < coded.size() && (coded[to].code >> 18) == (coded[from].code >> 18)) ++to;
            roots.push_back(Linear(&coded[from], &coded[0] + to, 17));
            from = to;
        }
        return JoinRoots(roots.data(), roots.data() + roots.size());
    }

    // depth first: a node, its first child's subtree, its second child's; returns the node's place
    int Lay(const Knot *k, std::vector<LinearBVHNode> *out) {
        const int here = (int)out->size();
        out->emplace_back();
        for (int a = 0; a < 3; ++a) { (*out)[here].bmin[a] = k->box.pMin[a]; (*out)[here].bmax[a] = k->box.pMax[a]; }
        if (k->count > 0) {
            if (k->count > kMaxStoredLeaf && stop.empty()) stop = "a leaf of 65536 primitives or more";
            (*out)[here].offset = k->first;
            (*out)[here].nPrimsAxis = 3u | ((uint32_t)k->count << 2);
        } else {
            (*out)[here].nPrimsAxis = (uint32_t)k->axis;      // an interior node holds no count
            Lay(k->kid[0], out);
            const int second = Lay(k->kid[1], out);
            (*out)[here].offset = second;
        }
        return here;
    }
};

// "" or why the reference's build stops
std::string Build(const std::vector<B3> &boxes, int how, int leafCap, Flat *flat) {
    flat->nodes.clear(); flat->sequence.clear();
    if (boxes.empty()) return "";
    Grower g;
    g.leafCap = std::min(255, leafCap);
    g.how = (How)how;
    std::vector<Item> items(boxes.size());
    for (size_t i = 0; i < boxes.size(); ++i) items[i] = Item{(uint32_t)i, boxes[i], .5f * boxes[i].pMin + .5f * boxes[i].pMax};
    const Knot *root = how == kMorton ? g.MortonBuild(items) : g.TopDown(items.data(), items.data() + items.size());
    if (g.stop.empty()) g.Lay(root, &flat->nodes);
    if (!g.stop.empty()) { flat->nodes.clear(); return g.stop; }
    flat->sequence = g.sequence;
    return "";
}

// A baked scene, with or without object instances: every aggregate's bvhold tree sits in an oracle BVH object (same node layout),
// whose primitive tests number a hit by the aggregate's place and the ordered position (top level first, then object 0, 1, ...)
struct SceneRef {
    Scene scene;
    std::vector<BVH> objectBvh;
    BVH bvh;
};

// The stack walk of one aggregate, closest hit (hit != null) or any hit: a node is fetched and its box tested; a leaf's
// primitives are tested in order; at an interior node the child on the ray's near side of the split axis goes first and the
// other waits on a stack of 64.  The counters: fetched, entered and leaf nodes of either kind of walk.
bool Walk(const BVH &agg, const Ray &ray, SurfaceInteraction *hit, Counters &ctr) {
    if (agg.nodes.empty()) return false;
    const bool anyHit = hit == nullptr;
    const V3 inv(1 / ray.d.x, 1 / ray.d.y, 1 / ray.d.z);
    const int backwards[3] = {inv.x < 0, inv.y < 0, inv.z < 0};
    int waiting[64], nWaiting = 0;
    bool found = false;
    for (int at = 0;;) {
        const LinearBVHNode &node = agg.nodes[at];
        ++(anyHit ? ctr.nodesFetchedP : ctr.nodesFetched);
        bool descend = false;
        if (BVH::SlabTest(&node, ray, inv, backwards)) {
            ++(anyHit ? ctr.nodesEnteredP : ctr.nodesEntered);
            if (node.IsLeaf()) {
                ++(anyHit ? ctr.leavesEnteredP : ctr.leavesEntered);
                for (uint32_t i = 0; i < node.nPrimitives(); ++i) {
                    if (anyHit) { if (agg.PrimIntersectP(node.offset + i, ray, ctr)) return true; }
                    else if (agg.PrimIntersect(node.offset + i, ray, hit, ctr)) found = true;
                }
            } else {
                const int near = backwards[node.SplitAxis()] ? node.offset : at + 1;
                waiting[nWaiting++] = backwards[node.SplitAxis()] ? at + 1 : node.offset;
                at = near;
                descend = true;
            }
        }
        if (descend) continue;
        if (nWaiting == 0) break;
        at = waiting[--nWaiting];
    }
    return found;
}

// the aggregate's bvhold tree in place of the oracle's own (an object's walk inside an instance is the oracle's BVH walk over
// these nodes: the same steps and the same counters as Walk)
std::string Rebuild(BVH *agg, size_t n, int how, int leafCap) {
    std::vector<B3> b(n);
    for (size_t i = 0; i < n; ++i) b[i] = agg->PrimWorldBound((uint32_t)i);
    Flat t;
    const std::string stop = Build(b, how, leafCap, &t);
    if (!stop.empty()) return stop;
    agg->nodes = t.nodes;
    agg->primOrder = t.sequence;
    return "";
}

}  // namespace

extern "C" {

const char *bvholdref_last_error() { return g_err.c_str(); }

// sizes[0..1] = nodes, primitives; null (bvholdref_last_error) where the reference's build stops
void *bvholdref_build(size_t n, const float *bmin, const float *bmax, int method, int maxPrims, uint32_t sizes[2]) {
    std::vector<B3> b(n);
    for (size_t i = 0; i < n; ++i) {
        b[i].pMin = V3(bmin[3 * i], bmin[3 * i + 1], bmin[3 * i + 2]);
        b[i].pMax = V3(bmax[3 * i], bmax[3 * i + 1], bmax[3 * i + 2]);
    }
    Flat *t = new Flat();
    const std::string stop = Build(b, method, maxPrims, t);
    if (!stop.empty()) { g_err = stop; delete t; return nullptr; }
    sizes[0] = (uint32_t)t->nodes.size(); sizes[1] = (uint32_t)t->sequence.size();
    return t;
}
void bvholdref_copy(void *h, void *nodes32, uint32_t *order) {
    const Flat *t = (const Flat *)h;
    if (nodes32 && !t->nodes.empty()) memcpy(nodes32, t->nodes.data(), t->nodes.size() * 32);
    if (order && !t->sequence.empty()) memcpy(order, t->sequence.data(), t->sequence.size() * 4);
}
void bvholdref_free(void *h) { delete (Flat *)h; }

void *bvholdref_scene_load(const char *path, int method, int maxPrims) {
    SceneRef *r = new SceneRef();
    std::string err;
    if (!LoadScene(path, &r->scene, &err)) { g_err = err; delete r; return nullptr; }
    const size_t nObj = r->scene.objectPrims.size();
    r->objectBvh.resize(nObj);
    uint32_t base = (uint32_t)r->scene.prims.size();
    for (size_t o = 0; o < nObj; ++o) {
        r->objectBvh[o].Build(&r->scene, &r->scene.objectPrims[o], &r->objectBvh, base);
        const std::string stop = Rebuild(&r->objectBvh[o], r->scene.objectPrims[o].size(), method, maxPrims);
        if (!stop.empty()) { g_err = stop; delete r; return nullptr; }
        base += (uint32_t)r->scene.objectPrims[o].size();
    }
    r->bvh.Build(&r->scene, &r->scene.prims, &r->objectBvh, 0);
    const std::string stop = Rebuild(&r->bvh, r->scene.prims.size(), method, maxPrims);      // (over the instances' bounds of the rebuilt objects)
    if (!stop.empty()) { g_err = stop; delete r; return nullptr; }
    return r;
}
void bvholdref_scene_free(void *h) { delete (SceneRef *)h; }
size_t bvholdref_scene_objects(void *h) { return ((SceneRef *)h)->objectBvh.size(); }
// object < 0: the top level
void bvholdref_scene_tree(void *h, int object, uint32_t sizes[2], void *nodes32, uint32_t *order) {
    const SceneRef *r = (const SceneRef *)h;
    const BVH &b = object < 0 ? r->bvh : r->objectBvh[object];
    sizes[0] = (uint32_t)b.nodes.size(); sizes[1] = (uint32_t)b.primOrder.size();
    if (nodes32 && !b.nodes.empty()) memcpy(nodes32, b.nodes.data(), b.nodes.size() * 32);
    if (order && !b.primOrder.empty()) memcpy(order, b.primOrder.data(), b.primOrder.size() * 4);
}
// the world bounds the aggregate's tree is built over, creation order (object < 0: the top level); returns how many
size_t bvholdref_scene_bounds(void *h, int object, float *bmin, float *bmax) {
    const SceneRef *r = (const SceneRef *)h;
    const BVH &b = object < 0 ? r->bvh : r->objectBvh[object];
    const size_t n = object < 0 ? r->scene.prims.size() : r->scene.objectPrims[object].size();
    if (bmin && bmax)
        for (size_t i = 0; i < n; ++i) {
            const B3 w = b.PrimWorldBound((uint32_t)i);
            for (int k = 0; k < 3; ++k) { bmin[3 * i + k] = w.pMin[k]; bmax[3 * i + k] = w.pMax[k]; }
        }
    return n;
}
// per ray: t, the ordered primitive over all aggregates (-1: none), the instance (-1: none), barycentrics and the counters
// nodes fetched, nodes entered, triangle tests, sphere tests, leaves entered (both levels together)
void bvholdref_intersect(void *h, size_t n, const float *o, const float *d, const float *tmax, float *tOut, int32_t *primOut, int32_t *instOut, float *bary,
                         uint64_t *counters5) {
    const SceneRef *r = (const SceneRef *)h;
    for (size_t i = 0; i < n; ++i) {
        Ray ray(V3(o[3 * i], o[3 * i + 1], o[3 * i + 2]), V3(d[3 * i], d[3 * i + 1], d[3 * i + 2]), tmax[i]);
        SurfaceInteraction si; Counters c;
        const bool hit = Walk(r->bvh, ray, &si, c);
        tOut[i] = ray.tMax; primOut[i] = hit ? si.ordered : -1; instOut[i] = hit ? si.inst : -1;
        bary[3 * i] = hit ? si.b0 : 0.f; bary[3 * i + 1] = hit ? si.b1 : 0.f; bary[3 * i + 2] = hit ? si.b2 : 0.f;
        counters5[5 * i] = c.nodesFetched; counters5[5 * i + 1] = c.nodesEntered; counters5[5 * i + 2] = c.triTests; counters5[5 * i + 3] = c.sphereTests;
        counters5[5 * i + 4] = c.leavesEntered;
    }
}
void bvholdref_occluded(void *h, size_t n, const float *o, const float *d, const float *tmax, uint8_t *occ, uint64_t *counters5) {
    const SceneRef *r = (const SceneRef *)h;
    for (size_t i = 0; i < n; ++i) {
        Ray ray(V3(o[3 * i], o[3 * i + 1], o[3 * i + 2]), V3(d[3 * i], d[3 * i + 1], d[3 * i + 2]), tmax[i]);
        Counters c;
        occ[i] = Walk(r->bvh, ray, nullptr, c) ? 1 : 0;
        counters5[5 * i] = c.nodesFetchedP; counters5[5 * i + 1] = c.nodesEnteredP; counters5[5 * i + 2] = c.triTestsP; counters5[5 * i + 3] = c.sphereTestsP;
        counters5[5 * i + 4] = c.leavesEnteredP;
    }
}

}  // extern "C"
