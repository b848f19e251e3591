// hprt host side — the stock pbrt-v3 BVH, Accelerator "bvhold" (see bvhold_builder.h for the contract).
#include <algorithm>
#include <limits>
#include "bvhold_builder.h"
#include "hprt_math.h"

namespace hprt {
namespace {

struct Box {
    float lo[3], hi[3];
    void reset() {      // Bounds3(): pMin = max, pMax = lowest
        for (int k = 0; k < 3; ++k) { lo[k] = std::numeric_limits<float>::max(); hi[k] = std::numeric_limits<float>::lowest(); }
    }
    void grow(const float *blo, const float *bhi) {      // Union(Bounds3, Bounds3): std::min / std::max per component
        for (int k = 0; k < 3; ++k) { lo[k] = sel_min(lo[k], blo[k]); hi[k] = sel_max(hi[k], bhi[k]); }
    }
    void growPoint(const float *p) { grow(p, p); }       // Union(Bounds3, Point3)
    float area() const {                                 // Bounds3::SurfaceArea, geometry.h:946-949
        float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
        return 2 * (dx * dy + dx * dz + dy * dz);
    }
    int maximumExtent() const {                          // geometry.h:956-964
        float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
        if (dx > dy && dx > dz) return 0;
        else if (dy > dz) return 1;
        else return 2;
    }
};

std::string LeafTooLarge(uint32_t count) {
    return "bvhold: a leaf of " + std::to_string(count) + " primitives; the reference stores fewer than " + std::to_string(kBvhOldMaxLeaf) +
           " (accelerators/bvhOld.cpp:648)";
}

std::string BadBucket() {
    return "bvhold: a centroid falls outside the 12 SAH buckets (bounds that are not finite, or whose sum overflows); the reference's build "
           "stops there (accelerators/bvhOld.cpp:331-332, :585-586)";
}

constexpr int kBuckets = 12;
// int b = nBuckets * offset; if (b == nBuckets) b = nBuckets - 1 (:327-330, :581-584), without converting what an int cannot
// hold: a NaN, or a product outside (-1, 13), gives -1, which the callers refuse as the reference's CHECK_GE / CHECK_LT
int BucketIndex(float scaled) {
    if (!(scaled > -1.f && scaled < (float)(kBuckets + 1))) return -1;
    const int b = (int)scaled;
    return b == kBuckets ? kBuckets - 1 : b;
}
struct Bucket { int count = 0; Box bounds; Bucket() { bounds.reset(); } };

// cost[i] of splitting after bucket i, base + (count0 * SA0 + count1 * SA1) / SA (:338-355, :591-607); the first minimum
int CheapestBucket(const Bucket *buckets, const Box &bounds, float base, float *cheapestOut) {
    float cost[kBuckets - 1];
    for (int i = 0; i < kBuckets - 1; ++i) {
        Box b0, b1; b0.reset(); b1.reset();
        int count0 = 0, count1 = 0;
        for (int j = 0; j <= i; ++j) { b0.grow(buckets[j].bounds.lo, buckets[j].bounds.hi); count0 += buckets[j].count; }
        for (int j = i + 1; j < kBuckets; ++j) { b1.grow(buckets[j].bounds.lo, buckets[j].bounds.hi); count1 += buckets[j].count; }
        cost[i] = base + (count0 * b0.area() + count1 * b1.area()) / bounds.area();
    }
    float cheapest = cost[0];
    int cutBucket = 0;
    for (int i = 1; i < kBuckets - 1; ++i)
        if (cost[i] < cheapest) { cheapest = cost[i]; cutBucket = i; }
    *cheapestOut = cheapest;
    return cutBucket;
}

struct TempNode { Box box; int child[2]; uint32_t axis, first, count; };      // count > 0: a leaf; child < 0: ~treelet (hlbvh)

// BVHPrimitiveInfoOld (:48-59)
struct PrimInfo { uint32_t primitiveNumber; float lo[3], hi[3], centroid[3]; };

struct Recursive {
    std::vector<PrimInfo> info;
    std::vector<TempNode> tmp;
    std::vector<uint32_t> *ordered;
    int method, maxPrimsInNode;
    std::string refused;

    int leaf(int node, int start, int end, const Box &bounds) {
        const uint32_t count = (uint32_t)(end - start);
        if (count >= kBvhOldMaxLeaf && refused.empty()) refused = LeafTooLarge(count);
        TempNode &nd = tmp[node];
        nd.box = bounds; nd.child[0] = nd.child[1] = -1; nd.axis = 3; nd.first = (uint32_t)ordered->size(); nd.count = count;
        for (int i = start; i < end; ++i) ordered->push_back(info[i].primitiveNumber);
        return node;
    }
    // recursiveBuild, :238-404
    int build(int start, int end) {
        const int node = (int)tmp.size();
        tmp.push_back(TempNode());
        Box bounds; bounds.reset();
        for (int i = start; i < end; ++i) bounds.grow(info[i].lo, info[i].hi);
        const int nPrimitives = end - start;
        if (nPrimitives == 1) return leaf(node, start, end, bounds);
        Box centres; centres.reset();
        for (int i = start; i < end; ++i) centres.growPoint(info[i].centroid);
        const int dim = centres.maximumExtent();
        int mid = (start + end) / 2;
        if (centres.hi[dim] == centres.lo[dim]) return leaf(node, start, end, bounds);
        PrimInfo *const first = info.data() + start, *const last = info.data() + end;      // plain pointers, as the reference passes
        auto equalCounts = [&] {
            mid = (start + end) / 2;
            std::nth_element(first, &info[mid], last, [dim](const PrimInfo &a, const PrimInfo &b) { return a.centroid[dim] < b.centroid[dim]; });
        };
        switch (method) {
            case BVHOLD_MIDDLE: {
                const float centre = (centres.lo[dim] + centres.hi[dim]) / 2;
                PrimInfo *split = std::partition(first, last, [dim, centre](const PrimInfo &pi) { return pi.centroid[dim] < centre; });
                mid = (int)(split - &info[0]);
                if (mid != start && mid != end) break;
                equalCounts();      // a one-sided partition falls through to EqualCounts (:290-294)
                break;
            }
            case BVHOLD_EQUAL: equalCounts(); break;
            case BVHOLD_SAH:
            default: {
                if (nPrimitives <= 2) { equalCounts(); break; }
                const float cmin = centres.lo[dim], cmax = centres.hi[dim];
                // nBuckets * centres.Offset(centroid)[dim]: Offset divides where pMax > pMin, which holds on dim
                auto bucketOf = [dim, cmin, cmax](const PrimInfo &pi) {
                    float o = pi.centroid[dim] - cmin;
                    if (cmax > cmin) o /= cmax - cmin;
                    return BucketIndex(kBuckets * o);
                };
                Bucket buckets[kBuckets];
                for (int i = start; i < end; ++i) {
                    const int b = bucketOf(info[i]);
                    if (b < 0 || b >= kBuckets) {      // CHECK_GE / CHECK_LT, :331-332
                        if (refused.empty()) refused = BadBucket();
                        return leaf(node, start, end, bounds);
                    }
                    buckets[b].count++;
                    buckets[b].bounds.grow(info[i].lo, info[i].hi);
                }
                float cheapest;
                const int cutBucket = CheapestBucket(buckets, bounds, 1, &cheapest);
                const float asLeaf = nPrimitives;
                if (nPrimitives > maxPrimsInNode || cheapest < asLeaf) {
                    PrimInfo *split = std::partition(first, last, [&](const PrimInfo &pi) { return bucketOf(pi) <= cutBucket; });
                    mid = (int)(split - &info[0]);
                } else return leaf(node, start, end, bounds);
                break;
            }
        }
        // the second child first: see the header
        const int c1 = build(mid, end);
        const int c0 = build(start, mid);
        TempNode &nd = tmp[node];
        nd.child[0] = c0; nd.child[1] = c1; nd.axis = (uint32_t)dim; nd.count = 0; nd.first = 0;
        nd.box = tmp[c0].box; nd.box.grow(tmp[c1].box.lo, tmp[c1].box.hi);      // Union(c0->bounds, c1->bounds), :76
        return node;
    }
};

void PutNode(BvhNode *ln, const Box &box, int32_t offset, uint32_t countAxis) {
    for (int k = 0; k < 3; ++k) { ln->bmin[k] = box.lo[k]; ln->bmax[k] = box.hi[k]; }
    ln->offset = offset; ln->countAxis = countAxis;
}

// depth and leaves of a finished array (children follow their parents)
void Finish(BvhTree *out) {
    int depth = 0;
    (void)CheckBvhNodes(out->nodes.data(), (uint32_t)out->nodes.size(), 0xffffffffu, &depth);
    out->maxDepth = depth;
    out->nLeaves = 0;
    for (const BvhNode &n : out->nodes) out->nLeaves += (n.countAxis & 3u) == 3u;
}

}  // namespace

namespace hlbvh {

void CentroidBounds(size_t n, const float *bmin, const float *bmax, float lo[3], float hi[3]) {
    Box b; b.reset();
    for (size_t i = 0; i < n; ++i) {
        float c[3];
        for (int k = 0; k < 3; ++k) c[k] = .5f * bmin[3 * i + k] + .5f * bmax[3 * i + k];
        b.growPoint(c);
    }
    for (int k = 0; k < 3; ++k) { lo[k] = b.lo[k]; hi[k] = b.hi[k]; }
}

// ten bits, each moved to every third position; 1024 (an offset of exactly one) counts as 1023 (:109-132)
static uint32_t SpreadBits10(uint32_t x) {
    if (x == 1024u) x = 1023u;
    x = (x | (x << 16)) & 0x30000ffu;
    x = (x | (x << 8)) & 0x300f00fu;
    x = (x | (x << 4)) & 0x30c30c3u;
    x = (x | (x << 2)) & 0x9249249u;
    return x;
}

uint32_t MortonCode(const float cen[3], const float lo[3], const float hi[3]) {
    uint32_t q[3];
    for (int k = 0; k < 3; ++k) {
        float o = cen[k] - lo[k];
        if (hi[k] > lo[k]) o /= hi[k] - lo[k];
        // the truncation of the device's conversion, spelled out: a value past 1024 (an extent that overflows) is 1024, a NaN or a
        // negative one 0.  Finite bounds give an offset in [0, 1], where this is the plain cast.
        const float s = o * 1024;
        q[k] = s >= 1024.f ? 1024u : (s > 0.f ? (uint32_t)s : 0u);
    }
    return (SpreadBits10(q[2]) << 2) | (SpreadBits10(q[1]) << 1) | SpreadBits10(q[0]);
}

// Any stable sort by the 30-bit code gives the reference's array (its own is an LSD radix sort, :141-182)
void SortMorton(std::vector<MortonPrim> *v) {
    std::stable_sort(v->begin(), v->end(), [](const MortonPrim &a, const MortonPrim &b) { return a.code < b.code; });
}

void FindTreelets(const MortonPrim *sorted, size_t n, std::vector<Treelet> *out) {
    out->clear();
    for (size_t first = 0; first < n;) {
        size_t past = first + 1;
        while (past < n && (sorted[past].code & kTreeletMask) == (sorted[first].code & kTreeletMask)) ++past;
        out->push_back(Treelet{(uint32_t)first, (uint32_t)(past - first), (uint32_t)(2 * first), 0u});
        first = past;
    }
}

std::string EmitTreelet(const MortonPrim *sorted, Treelet *t, int maxPrimsInNode, const float *bmin, const float *bmax, BvhNode *nodes) {
    struct Entry { uint32_t start, count; int bit; int parent; };      // parent: the interior node whose second child this is, or -1
    Entry stack[20];
    int sp = 0;
    BvhNode *out = nodes + t->nodeBase;
    uint32_t nOut = 0;
    stack[sp++] = Entry{t->start, t->count, kFirstBit, -1};
    while (sp > 0) {
        const Entry e = stack[--sp];
        const MortonPrim *mp = sorted + e.start;
        int bit = e.bit;
        // a level without a split is skipped (:498-503); the leaf test comes first (:483)
        while (!(bit == -1 || (int)e.count < maxPrimsInNode) && ((mp[0].code ^ mp[e.count - 1].code) & (1u << bit)) == 0) --bit;
        const uint32_t slot = nOut++;
        if (e.parent >= 0) out[e.parent].offset = (int32_t)slot;
        if (bit == -1 || (int)e.count < maxPrimsInNode) {
            if (e.count >= kBvhOldMaxLeaf) return LeafTooLarge(e.count);
            Box b; b.reset();
            for (uint32_t i = 0; i < e.count; ++i) b.grow(&bmin[3 * (size_t)mp[i].index], &bmax[3 * (size_t)mp[i].index]);
            PutNode(&out[slot], b, (int32_t)e.start, 3u | (e.count << 2));
            continue;
        }
        const uint32_t mask = 1u << bit;
        // the first primitive whose bit differs from the range's first (the codes are sorted): bisection
        const uint32_t side = mp[0].code & mask;
        uint32_t same = 0, other = e.count - 1;
        while (other - same > 1) {
            const uint32_t probe = same + (other - same) / 2;
            if ((mp[probe].code & mask) == side) same = probe; else other = probe;
        }
        const uint32_t cutAt = other;
        Box none; none.reset();
        PutNode(&out[slot], none, 0, (uint32_t)(bit % 3));
        stack[sp++] = Entry{e.start + cutAt, e.count - cutAt, bit - 1, (int)slot};
        stack[sp++] = Entry{e.start, cutAt, bit - 1, -1};
    }
    // interior boxes: Union(c0->bounds, c1->bounds) back to front, the first child next, the second at the stored offset
    for (uint32_t i = nOut; i-- > 0;) {
        if ((out[i].countAxis & 3u) == 3u) continue;
        const BvhNode &a = out[i + 1], &b = out[out[i].offset];
        for (int k = 0; k < 3; ++k) { out[i].bmin[k] = sel_min(a.bmin[k], b.bmin[k]); out[i].bmax[k] = sel_max(a.bmax[k], b.bmax[k]); }
    }
    t->nNodes = nOut;
    return "";
}

namespace {
struct Upper {
    const std::vector<Treelet> &treelets;
    const BvhNode *nodes;
    std::vector<uint32_t> roots;      // treeletRoots, as buildUpperSAH partitions it
    std::vector<TempNode> tmp;
    std::string refused;
    const BvhNode &root(uint32_t t) const { return nodes[treelets[t].nodeBase]; }

    // buildUpperSAH, :540-640; returns a tmp index or ~treelet
    int build(int start, int end) {
        if (end - start == 1) return ~(int)roots[start];
        const int node = (int)tmp.size();
        tmp.push_back(TempNode());
        Box bounds; bounds.reset();
        for (int i = start; i < end; ++i) bounds.grow(root(roots[i]).bmin, root(roots[i]).bmax);
        Box centres; centres.reset();
        for (int i = start; i < end; ++i) {
            const BvhNode &r = root(roots[i]);
            float c[3];
            for (int k = 0; k < 3; ++k) c[k] = (r.bmin[k] + r.bmax[k]) * 0.5f;
            centres.growPoint(c);
        }
        const int dim = centres.maximumExtent();
        const float cmin = centres.lo[dim], cmax = centres.hi[dim];
        if (cmax == cmin) {
            if (refused.empty())
                refused = "bvhold hlbvh: the centroids of " + std::to_string(end - start) + " treelet roots coincide on their widest axis; the reference's "
                          "upper SAH build is undefined there (accelerators/bvhOld.cpp:566)";
            return ~(int)roots[start];
        }
        auto bucketOf = [&](uint32_t t) {
            const BvhNode &r = root(t);
            const float centroid = (r.bmin[dim] + r.bmax[dim]) * 0.5f;
            return BucketIndex(kBuckets * ((centroid - cmin) / (cmax - cmin)));
        };
        Bucket buckets[kBuckets];
        for (int i = start; i < end; ++i) {
            const int b = bucketOf(roots[i]);
            if (b < 0 || b >= kBuckets) {      // CHECK_GE / CHECK_LT, :585-586
                if (refused.empty()) refused = BadBucket();
                return ~(int)roots[start];
            }
            buckets[b].count++;
            buckets[b].bounds.grow(root(roots[i]).bmin, root(roots[i]).bmax);
        }
        float cheapest;
        const int cutBucket = CheapestBucket(buckets, bounds, .125f, &cheapest);
        uint32_t *split = std::partition(roots.data() + start, roots.data() + end, [&](uint32_t t) { return bucketOf(t) <= cutBucket; });
        const int mid = (int)(split - roots.data());
        const int c0 = build(start, mid), c1 = build(mid, end);      // (the ranges are disjoint and nothing is numbered here: either order)
        TempNode &nd = tmp[node];
        nd.child[0] = c0; nd.child[1] = c1; nd.axis = (uint32_t)dim; nd.count = 0; nd.first = 0;
        const auto lo = [&](int c) { return c < 0 ? root((uint32_t)~c).bmin : tmp[c].box.lo; };
        const auto hi = [&](int c) { return c < 0 ? root((uint32_t)~c).bmax : tmp[c].box.hi; };
        for (int k = 0; k < 3; ++k) { nd.box.lo[k] = sel_min(lo(c0)[k], lo(c1)[k]); nd.box.hi[k] = sel_max(hi(c0)[k], hi(c1)[k]); }
        return node;
    }
    // flattenBVHTree over the upper nodes; a treelet's preorder array is copied, its interior offsets moved to its place
    int flatten(int c, std::vector<BvhNode> *out) {
        const int myOffset = (int)out->size();
        if (c < 0) {
            const Treelet &t = treelets[(uint32_t)~c];
            for (uint32_t i = 0; i < t.nNodes; ++i) {
                BvhNode n = nodes[t.nodeBase + i];
                if ((n.countAxis & 3u) != 3u) n.offset += myOffset;
                out->push_back(n);
            }
            return myOffset;
        }
        out->push_back(BvhNode());
        PutNode(&(*out)[myOffset], tmp[c].box, 0, tmp[c].axis);
        flatten(tmp[c].child[0], out);
        const int second = flatten(tmp[c].child[1], out);
        (*out)[myOffset].offset = second;
        return myOffset;
    }
};
}  // namespace

std::string Assemble(const MortonPrim *sorted, size_t n, const std::vector<Treelet> &treelets, const BvhNode *nodes, BvhTree *out) {
    out->nodes.clear(); out->primOrder.clear(); out->maxDepth = 0; out->nLeaves = 0;
    if (n == 0) return "";
    Upper up{treelets, nodes, {}, {}, ""};
    up.roots.resize(treelets.size());
    size_t total = 0;
    for (size_t t = 0; t < treelets.size(); ++t) { up.roots[t] = (uint32_t)t; total += treelets[t].nNodes; }
    const int root = up.build(0, (int)treelets.size());
    if (!up.refused.empty()) return up.refused;
    out->nodes.reserve(total + treelets.size());
    up.flatten(root, &out->nodes);
    out->primOrder.resize(n);
    for (size_t i = 0; i < n; ++i) out->primOrder[i] = sorted[i].index;
    Finish(out);
    return "";
}

}  // namespace hlbvh

std::string BuildBvhOld(size_t n, const float *bmin, const float *bmax, const BvhOldParams &params, BvhTree *out) {
    out->nodes.clear(); out->primOrder.clear(); out->maxDepth = 0; out->nLeaves = 0;
    if (n == 0) return "";
    const int maxPrimsInNode = std::min(255, (int)params.maxNodePrims);      // :187
    if (params.splitMethod == BVHOLD_HLBVH) {
        using namespace hlbvh;
        float lo[3], hi[3];
        CentroidBounds(n, bmin, bmax, lo, hi);
        std::vector<MortonPrim> mp(n);
        for (size_t i = 0; i < n; ++i) {
            float c[3];
            for (int k = 0; k < 3; ++k) c[k] = .5f * bmin[3 * i + k] + .5f * bmax[3 * i + k];
            mp[i].index = (uint32_t)i;
            mp[i].code = MortonCode(c, lo, hi);
        }
        SortMorton(&mp);
        std::vector<Treelet> treelets;
        FindTreelets(mp.data(), n, &treelets);
        std::vector<BvhNode> nodes(2 * n);
        for (Treelet &t : treelets) {
            const std::string refused = EmitTreelet(mp.data(), &t, maxPrimsInNode, bmin, bmax, nodes.data());
            if (!refused.empty()) return refused;
        }
        return Assemble(mp.data(), n, treelets, nodes.data(), out);
    }
    Recursive r;
    r.ordered = &out->primOrder; r.method = params.splitMethod; r.maxPrimsInNode = maxPrimsInNode;
    r.info.resize(n);
    for (size_t i = 0; i < n; ++i) {
        PrimInfo &pi = r.info[i];
        pi.primitiveNumber = (uint32_t)i;
        for (int k = 0; k < 3; ++k) { pi.lo[k] = bmin[3 * i + k]; pi.hi[k] = bmax[3 * i + k]; pi.centroid[k] = .5f * pi.lo[k] + .5f * pi.hi[k]; }
    }
    r.tmp.reserve(2 * n);
    out->primOrder.reserve(n);
    r.build(0, (int)n);
    if (!r.refused.empty()) { out->nodes.clear(); out->primOrder.clear(); return r.refused; }
    // flattenBVHTree, :642-660 (iterative: the first child next, the second after the first child's subtree)
    out->nodes.resize(r.tmp.size());
    struct Visit { int tnode, parentSlot; };
    std::vector<Visit> vs;
    vs.push_back(Visit{0, -1});
    int next = 0;
    while (!vs.empty()) {
        const Visit v = vs.back(); vs.pop_back();
        const TempNode &t = r.tmp[v.tnode];
        const int slot = next++;
        if (v.parentSlot >= 0) out->nodes[v.parentSlot].offset = slot;
        if (t.count) PutNode(&out->nodes[slot], t.box, (int32_t)t.first, 3u | (t.count << 2));
        else {
            PutNode(&out->nodes[slot], t.box, 0, t.axis);
            vs.push_back(Visit{t.child[1], slot});
            vs.push_back(Visit{t.child[0], -1});
        }
    }
    Finish(out);
    return "";
}

}  // namespace hprt
