// hprt — the HLBVH form of Accelerator "bvhold" built on gfx950 (HLBVHBuild / emitLBVH, accelerators/bvhOld.cpp:406-538): the
// first build of this library whose bulk runs on the GPU.  A translation unit of its own with a pinned CUID (build.py), so that
// the other code objects stay byte for byte what they were.  The tree equals bvhold_builder.cpp's byte for byte: every step is
// integer work, a float operation in source order (-ffp-contract=off, hipcc's correctly rounded float division) or a min / max
// whose result does not depend on the order.
//
//   k_hlbvh_centroids   per-workgroup min / max of the centroids; the host finishes the at most kCentroidBlocks partials
//   k_hlbvh_morton      Bounds3::Offset, * 1024, truncation, bit spreading: {code, index}
//   k_radix_hist / k_radix_scan / k_radix_scatter   a stable LSD radix sort of the 30 bits, 4 passes of 8 bits
//   k_hlbvh_treelets / k_hlbvh_compact   where the top 12 bits change, and the starts compacted (at most 4,096)
//   k_hlbvh_emit        one lane per treelet: emitLBVH with an explicit stack in LDS, preorder, treelet-relative offsets
//   k_hlbvh_pack        the treelets' node arrays moved next to each other for one download
//
// Every dependency between workgroups is a kernel boundary: no kernel waits for another workgroup.  Every index a kernel
// forms is checked against the array it goes into.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>
#include "../../../include/hprt.h"
#include "../hlbvh_build_device.h"
#include "cost_session.h"

namespace hprt {
namespace {

using hlbvh::MortonPrim;
using hlbvh::Treelet;

constexpr uint32_t kBlock = 256;                       // four waves
constexpr uint32_t kWaves = kBlock / kWave;
constexpr uint32_t kCentroidBlocks = 1024;             // grid-stride: at most this many partials
constexpr uint32_t kRadixBits = 8, kDigits = 1u << kRadixBits, kPasses = 4;      // 4 * 8 >= 30
constexpr uint32_t kItems = 8, kTile = kBlock * kItems;                         // keys per workgroup and pass
constexpr uint32_t kScanItems = 8;                     // table entries per thread and step of k_radix_scan
constexpr uint32_t kNoStart = 0xffffffffu;
constexpr uint32_t kEmitBlock = kWave;                 // one wave: 4,096 lanes spread over 64 workgroups
constexpr uint32_t kEmitStack = 20;                    // emitLBVH holds at most 19 entries (18 levels below bit 17, two children at the last)
static_assert(kDigits == kBlock, "k_radix_*: one digit per thread");

// LDS per workgroup, as the kernels declare it (tests/test_gpu_bvhold.py reads these lines and the code object's metadata)
constexpr uint32_t kLdsCentroids = 6 * kWaves * 4;                       // k_hlbvh_centroids
constexpr uint32_t kLdsHist = kDigits * 4;                               // k_radix_hist
constexpr uint32_t kLdsScan = kWaves * 4;                                // k_radix_scan, k_hlbvh_compact
constexpr uint32_t kLdsScatter = kDigits * 4 + kWaves * kDigits * 4;     // k_radix_scatter
constexpr uint32_t kLdsEmit = 3 * kEmitStack * kEmitBlock * 4;           // k_hlbvh_emit
static_assert(kLdsCentroids == 96, "LDS k_hlbvh_centroids");
static_assert(kLdsHist == 1024, "LDS k_radix_hist");
static_assert(kLdsScan == 16, "LDS k_radix_scan k_hlbvh_compact");
static_assert(kLdsScatter == 5120, "LDS k_radix_scatter");
static_assert(kLdsEmit == 15360, "LDS k_hlbvh_emit");

__device__ inline float d_min(float a, float b) { return (b < a) ? b : a; }      // std::min / std::max, operand for operand
__device__ inline float d_max(float a, float b) { return (a < b) ? b : a; }

__global__ __launch_bounds__(kBlock) void k_hlbvh_centroids(const float *__restrict__ bmin, const float *__restrict__ bmax, uint32_t n,
                                                            float *__restrict__ partial) {
    __shared__ float sPart[6 * kWaves];
    float lo[3], hi[3];
    for (int k = 0; k < 3; ++k) { lo[k] = 3.402823466e+38f; hi[k] = -3.402823466e+38f; }
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        for (int k = 0; k < 3; ++k) {
            const float c = .5f * bmin[3 * (size_t)i + k] + .5f * bmax[3 * (size_t)i + k];
            lo[k] = d_min(lo[k], c); hi[k] = d_max(hi[k], c);
        }
    }
    for (int k = 0; k < 3; ++k)
        for (uint32_t d = kWave / 2; d > 0; d >>= 1) { lo[k] = d_min(lo[k], __shfl_down(lo[k], d)); hi[k] = d_max(hi[k], __shfl_down(hi[k], d)); }
    const uint32_t wave = threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0)
        for (int k = 0; k < 3; ++k) { sPart[6 * wave + k] = lo[k]; sPart[6 * wave + 3 + k] = hi[k]; }
    __syncthreads();
    if (threadIdx.x < 6) {
        float v = sPart[threadIdx.x];
        for (uint32_t w = 1; w < kWaves; ++w) v = threadIdx.x < 3 ? d_min(v, sPart[6 * w + threadIdx.x]) : d_max(v, sPart[6 * w + threadIdx.x]);
        partial[6 * blockIdx.x + threadIdx.x] = v;
    }
}

__device__ inline uint32_t SpreadBits10(uint32_t x) {      // bvhOld.cpp:109-132
    if (x == (1u << 10)) --x;
    x = (x | (x << 16)) & 0x30000ffu;
    x = (x | (x << 8)) & 0x300f00fu;
    x = (x | (x << 4)) & 0x30c30c3u;
    x = (x | (x << 2)) & 0x9249249u;
    return x;
}

struct F3 { float v[3]; };

__global__ __launch_bounds__(kBlock) void k_hlbvh_morton(const float *__restrict__ bmin, const float *__restrict__ bmax, uint32_t n, F3 lo, F3 hi,
                                                         MortonPrim *__restrict__ out) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    uint32_t q[3];
    for (int k = 0; k < 3; ++k) {
        const float c = .5f * bmin[3 * (size_t)i + k] + .5f * bmax[3 * (size_t)i + k];
        float o = c - lo.v[k];
        if (hi.v[k] > lo.v[k]) o /= hi.v[k] - lo.v[k];
        q[k] = (uint32_t)(o * 1024);
        if (q[k] > 1024u) q[k] = 1024u;      // (never for finite input: Offset is in [0, 1]; keeps the code inside its 30 bits)
    }
    MortonPrim mp;
    mp.code = (SpreadBits10(q[2]) << 2) | (SpreadBits10(q[1]) << 1) | SpreadBits10(q[0]);
    mp.index = i;
    out[i] = mp;
}

// table[digit * nWG + workgroup]: the digit's count in the workgroup's tile
__global__ __launch_bounds__(kBlock) void k_radix_hist(const MortonPrim *__restrict__ in, uint32_t n, uint32_t shift, uint32_t nWG,
                                                       uint32_t *__restrict__ table) {
    __shared__ uint32_t sHist[kDigits];
    sHist[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * kTile;
    for (uint32_t r = 0; r < kItems; ++r) {
        const uint32_t i = base + r * kBlock + threadIdx.x;
        if (i < n) atomicAdd(&sHist[(in[i].code >> shift) & (kDigits - 1)], 1u);
    }
    __syncthreads();
    if (blockIdx.x < nWG) table[(size_t)threadIdx.x * nWG + blockIdx.x] = sHist[threadIdx.x];
}

// The inclusive scan of v over the workgroup's threads; *total: the sum over all of them.  sWave: kWaves words of LDS.
__device__ inline uint32_t BlockInclusiveScan(uint32_t v, uint32_t *sWave, uint32_t *total) {
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    uint32_t s = v;
    for (uint32_t d = 1; d < kWave; d <<= 1) { const uint32_t u = __shfl_up(s, d); if (lane >= d) s += u; }
    __syncthreads();      // (the previous use of sWave is over)
    if (lane == kWave - 1) sWave[wave] = s;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t w = 0; w < kWaves; ++w) { const uint32_t t = sWave[w]; all += t; if (w < wave) before += t; }
    *total = all;
    return s + before;
}

// Exclusive scan of the whole table in place, one workgroup: the digit-major order makes it the keys' destinations
__global__ __launch_bounds__(kBlock) void k_radix_scan(uint32_t *__restrict__ table, uint32_t len) {
    __shared__ uint32_t sWave[kWaves];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < len; base += kBlock * kScanItems) {
        const uint32_t first = base + threadIdx.x * kScanItems;
        uint32_t v[kScanItems], sum = 0;
        for (uint32_t k = 0; k < kScanItems; ++k) { v[k] = first + k < len ? table[first + k] : 0u; sum += v[k]; }
        uint32_t total;
        uint32_t run = carry + BlockInclusiveScan(sum, sWave, &total) - sum;
        for (uint32_t k = 0; k < kScanItems; ++k) { if (first + k < len) table[first + k] = run; run += v[k]; }
        carry += total;
    }
}

// Stable: within a wave a key's rank among the keys of its digit comes from one ballot per digit bit; the waves' digit
// counts sit in LDS and are taken in wave order; the rounds of a tile run in order
__global__ __launch_bounds__(kBlock) void k_radix_scatter(const MortonPrim *__restrict__ in, MortonPrim *__restrict__ out, uint32_t n, uint32_t shift,
                                                          uint32_t nWG, const uint32_t *__restrict__ table) {
    __shared__ uint32_t sBase[kDigits];
    __shared__ uint32_t sCount[kWaves][kDigits];
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    sBase[threadIdx.x] = blockIdx.x < nWG ? table[(size_t)threadIdx.x * nWG + blockIdx.x] : n;
    for (uint32_t w = 0; w < kWaves; ++w) sCount[w][threadIdx.x] = 0;
    const uint32_t base = blockIdx.x * kTile;
    for (uint32_t r = 0; r < kItems; ++r) {
        __syncthreads();      // sBase and the zeroed sCount of this round
        const uint32_t i = base + r * kBlock + threadIdx.x;
        const bool valid = i < n;
        MortonPrim mp; mp.code = 0; mp.index = 0;
        if (valid) mp = in[i];
        const uint32_t digit = (mp.code >> shift) & (kDigits - 1);
        unsigned long long peers = __ballot(valid);
        for (uint32_t b = 0; b < kRadixBits; ++b) {
            const bool bit = (digit >> b) & 1u;
            const unsigned long long bal = __ballot(valid && bit);
            peers &= bit ? bal : ~bal;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
        if (valid && rank == 0) sCount[wave][digit] = (uint32_t)__popcll(peers);
        __syncthreads();
        if (valid) {
            uint32_t pos = sBase[digit] + rank;
            for (uint32_t w = 0; w < wave; ++w) pos += sCount[w][digit];
            if (pos < n) out[pos] = mp;
        }
        __syncthreads();
        uint32_t add = 0;
        for (uint32_t w = 0; w < kWaves; ++w) { add += sCount[w][threadIdx.x]; sCount[w][threadIdx.x] = 0; }
        sBase[threadIdx.x] += add;
    }
}

// starts[key]: the sorted position at which the 12-bit key first appears (kNoStart: never)
__global__ __launch_bounds__(kBlock) void k_hlbvh_treelets(const MortonPrim *__restrict__ sorted, uint32_t n, uint32_t *__restrict__ starts) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t key = (sorted[i].code & hlbvh::kTreeletMask) >> 18;
    if (key < hlbvh::kMaxTreelets && (i == 0 || ((sorted[i - 1].code & hlbvh::kTreeletMask) >> 18) != key)) starts[key] = i;
}

// One workgroup: the starts that are there, in key order (which is the sorted order); compact[kMaxTreelets] = how many
__global__ __launch_bounds__(kBlock) void k_hlbvh_compact(const uint32_t *__restrict__ starts, uint32_t *__restrict__ compact) {
    __shared__ uint32_t sWave[kWaves];
    constexpr uint32_t per = hlbvh::kMaxTreelets / kBlock;
    uint32_t v[per], cnt = 0;
    for (uint32_t k = 0; k < per; ++k) { v[k] = starts[threadIdx.x * per + k]; cnt += v[k] != kNoStart; }
    uint32_t total;
    uint32_t pos = BlockInclusiveScan(cnt, sWave, &total) - cnt;
    for (uint32_t k = 0; k < per; ++k)
        if (v[k] != kNoStart && pos < hlbvh::kMaxTreelets) compact[pos++] = v[k];
    if (threadIdx.x == 0) compact[hlbvh::kMaxTreelets] = total;
}

struct alignas(16) Node32 { float bmin[3], bmax[3]; int32_t offset; uint32_t countAxis; };      // == BvhNode
static_assert(sizeof(Node32) == 32, "Node32 is BvhNode");

// emitLBVH (:476-538) for treelet t = the lane's number: nodes[2 * start ...] in preorder, interior offsets relative to the
// treelet, leaf offsets the sorted position; nNodes[t] = how many, 0 for a treelet left to the host (more than serialMax
// primitives, or a leaf the reference cannot store).  The stack is in LDS, [entry][lane]: no run-time-indexed private array.
__global__ __launch_bounds__(kEmitBlock) void k_hlbvh_emit(const MortonPrim *__restrict__ sorted, uint32_t n, const float *__restrict__ bmin,
                                                           const float *__restrict__ bmax, const uint32_t *__restrict__ compact, int maxPrimsInNode,
                                                           uint32_t serialMax, Node32 *__restrict__ nodes, uint32_t *__restrict__ nNodes) {
    __shared__ uint32_t sStart[kEmitStack][kEmitBlock], sCount[kEmitStack][kEmitBlock], sMeta[kEmitStack][kEmitBlock];      // meta: bit + 1 | (parent + 1) << 5
    const uint32_t lane = threadIdx.x;
    const uint32_t t = blockIdx.x * kEmitBlock + lane;
    const uint32_t nTreelets = compact[hlbvh::kMaxTreelets];
    if (t >= nTreelets || t >= hlbvh::kMaxTreelets) return;
    const uint32_t tStart = compact[t], tEnd = t + 1 < nTreelets ? compact[t + 1] : n;
    if (tStart >= tEnd || tEnd > n) { nNodes[t] = 0; return; }
    const uint32_t tCount = tEnd - tStart;
    if (tCount > serialMax) { nNodes[t] = 0; return; }
    Node32 *out = nodes + 2 * (size_t)tStart;
    const uint32_t cap = 2 * tCount;      // the treelet's share of the array (it needs 2 tCount - 1 at most)
    uint32_t nOut = 0, sp = 0;
    bool ok = true;
    sStart[0][lane] = tStart; sCount[0][lane] = tCount; sMeta[0][lane] = (uint32_t)(hlbvh::kFirstBit + 1);
    sp = 1;
    while (sp > 0 && ok) {
        --sp;
        const uint32_t eStart = sStart[sp][lane], eCount = sCount[sp][lane], meta = sMeta[sp][lane];
        int bit = (int)(meta & 31u) - 1;
        const int parent = (int)(meta >> 5) - 1;
        const MortonPrim *mp = sorted + eStart;
        const bool small = (int)eCount < maxPrimsInNode;
        const uint32_t diff = mp[0].code ^ mp[eCount - 1].code;
        while (bit != -1 && !small && ((diff >> bit) & 1u) == 0) --bit;
        const uint32_t slot = nOut++;
        if (slot >= cap) { ok = false; break; }
        if (parent >= 0) out[parent].offset = (int32_t)slot;
        Node32 nd;
        if (bit == -1 || small) {
            if (eCount >= kBvhOldMaxLeaf) { ok = false; break; }
            for (int k = 0; k < 3; ++k) { nd.bmin[k] = 3.402823466e+38f; nd.bmax[k] = -3.402823466e+38f; }
            for (uint32_t i = 0; i < eCount; ++i) {
                const uint32_t p = mp[i].index;
                if (p >= n) { ok = false; break; }
                for (int k = 0; k < 3; ++k) { nd.bmin[k] = d_min(nd.bmin[k], bmin[3 * (size_t)p + k]); nd.bmax[k] = d_max(nd.bmax[k], bmax[3 * (size_t)p + k]); }
            }
            nd.offset = (int32_t)eStart; nd.countAxis = 3u | (eCount << 2);
            out[slot] = nd;
            continue;
        }
        const uint32_t mask = 1u << bit;
        // the first primitive whose bit differs from the range's first (the codes are sorted): bisection
        const uint32_t side = mp[0].code & mask;
        uint32_t same = 0, other = eCount - 1;
        while (same + 1 != other) {
            const uint32_t probe = (same + other) / 2;
            if ((mp[probe].code & mask) == side) same = probe; else other = probe;
        }
        const uint32_t cutAt = other;
        for (int k = 0; k < 3; ++k) { nd.bmin[k] = 0.f; nd.bmax[k] = 0.f; }
        nd.offset = 0; nd.countAxis = (uint32_t)(bit % 3);
        out[slot] = nd;
        if (sp + 2 > kEmitStack) { ok = false; break; }
        sStart[sp][lane] = eStart + cutAt; sCount[sp][lane] = eCount - cutAt; sMeta[sp][lane] = (uint32_t)bit | ((slot + 1u) << 5);      // bit - 1, + 1
        ++sp;
        sStart[sp][lane] = eStart; sCount[sp][lane] = cutAt; sMeta[sp][lane] = (uint32_t)bit;
        ++sp;
    }
    if (!ok) { nNodes[t] = 0; return; }
    // interior boxes back to front: Union(c0->bounds, c1->bounds), the first child next, the second at the stored offset
    for (uint32_t i = nOut; i-- > 0;) {
        Node32 nd = out[i];
        if ((nd.countAxis & 3u) == 3u) continue;
        const uint32_t second = (uint32_t)nd.offset;
        if (i + 1 >= nOut || second >= nOut) { nNodes[t] = 0; return; }
        const Node32 a = out[i + 1], b = out[second];
        for (int k = 0; k < 3; ++k) { nd.bmin[k] = d_min(a.bmin[k], b.bmin[k]); nd.bmax[k] = d_max(a.bmax[k], b.bmax[k]); }
        out[i] = nd;
    }
    nNodes[t] = nOut;
}

// place[t] = {source (2 * start), destination, count}: one workgroup per treelet
struct Place { uint32_t src, dst, count, pad; };
__global__ __launch_bounds__(kBlock) void k_hlbvh_pack(const Node32 *__restrict__ nodes, size_t nNodesSrc, const Place *__restrict__ place,
                                                       Node32 *__restrict__ packed, size_t nPacked) {
    const Place p = place[blockIdx.x];
    if ((size_t)p.src + p.count > nNodesSrc || (size_t)p.dst + p.count > nPacked) return;
    for (uint32_t i = threadIdx.x; i < p.count; i += kBlock) packed[(size_t)p.dst + i] = nodes[(size_t)p.src + i];
}

}  // namespace

struct HlbvhDevice : CostSession {      // hOut: the downloads (partials, treelet starts and node counts, the sorted array, the packed nodes)
    uint32_t serialMax = kHlbvhSerialTreeletDefault;
    Dev dMin, dMax, dKeysA, dKeysB, dTable, dSmall, dNodes, dPacked, dPlace;
};

int HlbvhDeviceCount(int *n, std::string *err) { return CostDeviceCount(n, err); }

int HlbvhDeviceCreate(int device, uint32_t serialTreeletMax, HlbvhDevice **out, std::string *err) {
    *out = nullptr;
    int n = 0;
    if (const int rc = CostDeviceCount(&n, err)) return rc;
    if (serialTreeletMax > kHlbvhSerialTreeletCap) {
        *err = "serial_treelet_max may only lower the compiled capacity (" + std::to_string(kHlbvhSerialTreeletCap) + ")";
        return HPRT_E_INVALID;
    }
    HlbvhDevice *d = new HlbvhDevice();
    d->serialMax = serialTreeletMax ? serialTreeletMax : kHlbvhSerialTreeletDefault;
    if (const int rc = d->Open(device, n, err)) { delete d; return rc; }
    *out = d;
    return HPRT_OK;
}

void HlbvhDeviceDestroy(HlbvhDevice *d) { CostSessionDestroy(d); }

int HlbvhDeviceBuild(HlbvhDevice *d, size_t nIn, const float *bmin, const float *bmax, int maxNodePrims, BvhTree *out, HprtBvhOldDeviceStats *stats,
                     std::string *err) {
    out->nodes.clear(); out->primOrder.clear(); out->maxDepth = 0; out->nLeaves = 0;
    if (nIn == 0) return HPRT_OK;
    if (nIn > kHlbvhMaxPrims) { *err = "hlbvh device build: more than 2^26 primitives"; return HPRT_E_UNSUPPORTED; }
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t n = (uint32_t)nIn;
    const int maxPrimsInNode = std::min(255, maxNodePrims);      // bvhOld.cpp:187
#define HL_TRY(x) COST_TRY("hlbvh build", x)
    HL_TRY(hipSetDevice(d->device));
    hipStream_t s = d->stream;
    uint64_t launches = 0;
    const uint32_t nBlocks = (n + kBlock - 1) / kBlock, nWG = (n + kTile - 1) / kTile;
    const uint32_t cBlocks = std::min(nBlocks, kCentroidBlocks);
    const size_t tableLen = (size_t)kDigits * nWG;
    constexpr uint32_t kT = hlbvh::kMaxTreelets;
    // dSmall: centroid partials | treelet starts by key | compacted starts and their count | node counts
    const size_t offPartial = 0, offStarts = Pad16((size_t)6 * kCentroidBlocks * 4), offCompact = offStarts + (size_t)kT * 4,
                 offCounts = offCompact + Pad16((size_t)(kT + 1) * 4), smallBytes = offCounts + (size_t)kT * 4;
    HL_TRY(d->dMin.reserve((size_t)n * 12)); HL_TRY(d->dMax.reserve((size_t)n * 12));
    HL_TRY(d->dKeysA.reserve((size_t)n * 8)); HL_TRY(d->dKeysB.reserve((size_t)n * 8));
    HL_TRY(d->dTable.reserve(tableLen * 4)); HL_TRY(d->dSmall.reserve(smallBytes));
    HL_TRY(d->dNodes.reserve((size_t)n * 64));
    HL_TRY(d->hOut.reserve(std::max<size_t>(smallBytes, (size_t)n * 8)));
    char *small = (char *)d->dSmall.p;
    const float *dMin = (const float *)d->dMin.p, *dMax = (const float *)d->dMax.p;
    MortonPrim *keysA = (MortonPrim *)d->dKeysA.p, *keysB = (MortonPrim *)d->dKeysB.p;
    HL_TRY(hipMemcpyAsync(d->dMin.p, bmin, (size_t)n * 12, hipMemcpyHostToDevice, s));
    HL_TRY(hipMemcpyAsync(d->dMax.p, bmax, (size_t)n * 12, hipMemcpyHostToDevice, s));

    // centroid bounds: the partials finish here (min and max do not depend on the order)
    hipLaunchKernelGGL(k_hlbvh_centroids, dim3(cBlocks), dim3(kBlock), 0, s, dMin, dMax, n, (float *)(small + offPartial));
    HL_TRY(hipGetLastError()); ++launches;
    HL_TRY(hipMemcpyAsync(d->hOut.p, small + offPartial, (size_t)6 * cBlocks * 4, hipMemcpyDeviceToHost, s));
    HL_TRY(hipStreamSynchronize(s));
    F3 lo, hi;
    {
        const float *p = (const float *)d->hOut.p;
        for (int k = 0; k < 3; ++k) { lo.v[k] = p[k]; hi.v[k] = p[3 + k]; }
        for (uint32_t b = 1; b < cBlocks; ++b)
            for (int k = 0; k < 3; ++k) { lo.v[k] = sel_min(lo.v[k], p[6 * b + k]); hi.v[k] = sel_max(hi.v[k], p[6 * b + 3 + k]); }
    }
    hipLaunchKernelGGL(k_hlbvh_morton, dim3(nBlocks), dim3(kBlock), 0, s, dMin, dMax, n, lo, hi, keysA);
    HL_TRY(hipGetLastError()); ++launches;

    // the sort: an even number of passes leaves the result in keysA
    for (uint32_t pass = 0; pass < kPasses; ++pass) {
        const MortonPrim *in = (pass & 1) ? keysB : keysA;
        MortonPrim *outKeys = (pass & 1) ? keysA : keysB;
        const uint32_t shift = pass * kRadixBits;
        hipLaunchKernelGGL(k_radix_hist, dim3(nWG), dim3(kBlock), 0, s, in, n, shift, nWG, (uint32_t *)d->dTable.p);
        HL_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_radix_scan, dim3(1), dim3(kBlock), 0, s, (uint32_t *)d->dTable.p, (uint32_t)tableLen);
        HL_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_radix_scatter, dim3(nWG), dim3(kBlock), 0, s, in, outKeys, n, shift, nWG, (const uint32_t *)d->dTable.p);
        HL_TRY(hipGetLastError());
        launches += 3;
    }
    static_assert(kPasses % 2 == 0, "the sorted array is keysA");

    // treelets
    HL_TRY(hipMemsetAsync(small + offStarts, 0xff, (size_t)kT * 4, s));
    hipLaunchKernelGGL(k_hlbvh_treelets, dim3(nBlocks), dim3(kBlock), 0, s, keysA, n, (uint32_t *)(small + offStarts));
    HL_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_hlbvh_compact, dim3(1), dim3(kBlock), 0, s, (const uint32_t *)(small + offStarts), (uint32_t *)(small + offCompact));
    HL_TRY(hipGetLastError());
    HL_TRY(hipMemsetAsync(small + offCounts, 0, (size_t)kT * 4, s));
    hipLaunchKernelGGL(k_hlbvh_emit, dim3(kT / kEmitBlock), dim3(kEmitBlock), 0, s, keysA, n, dMin, dMax, (const uint32_t *)(small + offCompact),
                       maxPrimsInNode, d->serialMax, (Node32 *)d->dNodes.p, (uint32_t *)(small + offCounts));
    HL_TRY(hipGetLastError());
    launches += 3;
    HL_TRY(hipMemcpyAsync(d->hOut.p, small + offCompact, smallBytes - offCompact, hipMemcpyDeviceToHost, s));
    HL_TRY(hipStreamSynchronize(s));
    // (copies: the staging buffer is reserved again below)
    const uint32_t *stagedCompact = (const uint32_t *)d->hOut.p, *stagedCounts = (const uint32_t *)((const char *)d->hOut.p + (offCounts - offCompact));
    const std::vector<uint32_t> hCompact(stagedCompact, stagedCompact + kT + 1), hCounts(stagedCounts, stagedCounts + kT);
    const uint32_t nTreelets = hCompact[kT];
    if (nTreelets == 0 || nTreelets > kT) { *err = "hlbvh build: the device reported " + std::to_string(nTreelets) + " treelets"; return HPRT_E_DEVICE; }
    std::vector<Treelet> treelets(nTreelets);
    std::vector<Place> place;
    size_t nPacked = 0, nHostNodes = 0;
    uint64_t treeletsHost = 0;
    for (uint32_t t = 0; t < nTreelets; ++t) {
        const uint32_t start = hCompact[t], end = t + 1 < nTreelets ? hCompact[t + 1] : n;
        if (start >= end || end > n || (t == 0 && start != 0) || hCounts[t] > 2 * (end - start)) { *err = "hlbvh build: malformed treelet table from the device"; return HPRT_E_DEVICE; }
        treelets[t] = Treelet{start, end - start, 0u, hCounts[t]};
        if (hCounts[t]) { place.push_back(Place{2 * start, (uint32_t)nPacked, hCounts[t], 0u}); treelets[t].nodeBase = (uint32_t)nPacked; nPacked += hCounts[t]; }
        else { ++treeletsHost; nHostNodes += 2 * (size_t)(end - start); }
    }
    // the treelets' nodes next to each other, then one download of them and one of the sorted array
    const size_t sortedBytes = Pad16((size_t)n * 8);
    HL_TRY(d->hOut.reserve(sortedBytes + nPacked * 32));
    if (!place.empty()) {
        HL_TRY(d->dPacked.reserve(nPacked * 32));
        HL_TRY(d->dPlace.reserve(place.size() * sizeof(Place)));
        HL_TRY(hipMemcpyAsync(d->dPlace.p, place.data(), place.size() * sizeof(Place), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_hlbvh_pack, dim3((uint32_t)place.size()), dim3(kBlock), 0, s, (const Node32 *)d->dNodes.p, (size_t)2 * n, (const Place *)d->dPlace.p,
                           (Node32 *)d->dPacked.p, nPacked);
        HL_TRY(hipGetLastError()); ++launches;
        HL_TRY(hipMemcpyAsync((char *)d->hOut.p + sortedBytes, d->dPacked.p, nPacked * 32, hipMemcpyDeviceToHost, s));
    }
    HL_TRY(hipMemcpyAsync(d->hOut.p, keysA, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    HL_TRY(hipStreamSynchronize(s));
#undef HL_TRY
    const MortonPrim *sorted = (const MortonPrim *)d->hOut.p;
    std::vector<BvhNode> nodes(nPacked + nHostNodes);
    if (nPacked) std::memcpy(nodes.data(), (const char *)d->hOut.p + sortedBytes, nPacked * 32);
    // the treelets one lane does not walk: emitted here, with the host builder's own function
    size_t hostBase = nPacked;
    for (Treelet &t : treelets) {
        if (t.nNodes) continue;
        t.nodeBase = (uint32_t)hostBase;
        hostBase += 2 * (size_t)t.count;
        const std::string refused = hlbvh::EmitTreelet(sorted, &t, maxPrimsInNode, bmin, bmax, nodes.data());
        if (!refused.empty()) { *err = refused; return HPRT_E_UNSUPPORTED; }
    }
    const std::string refused = hlbvh::Assemble(sorted, n, treelets, nodes.data(), out);
    if (!refused.empty()) { *err = refused; return HPRT_E_UNSUPPORTED; }
    if (stats) {
        stats->prims_sorted += n; stats->sort_passes += kPasses; stats->treelets += nTreelets; stats->treelets_host += treeletsHost; stats->launches += launches;
        stats->seconds_device += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    return HPRT_OK;
}

}  // namespace hprt
