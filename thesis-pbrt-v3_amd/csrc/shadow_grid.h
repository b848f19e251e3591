// hprt — the light-centred candidate grid of point-light shadow rays: six cube faces of R x R cells around the
// light, each cell a list of the triangles that a shadow ray seen from the light in that cell's directions could be reported to
// hit, nearest first.  k_shadow_grid (device/shadow_grid.hip) runs the walk's own triangle and leaf-box tests over the list of a
// ray's cell instead of walking the BVH.  Host only, no HIP runtime call; hprt_scene_create uploads the result.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace hprt {

// An entry's first word: ordered primitive index (< 2^28) | SG_SINGLE when the primitive's leaf holds that one triangle alone and
// its exact box is the min / max of the vertices (the WIDE_LEAF_BOXED | WIDE_LEAF_FIRST mark of the wide records' leaf references).
// Its second word: in the upper 16 bits those of the depth key, a non-negative float cut off below them (so a key never grows, and
// keys order as unsigned integers); in the lower 16 the part of the cell that the triangle's widened rectangle reaches, in
// sixteenths of the cell: u from bits 0-3 to bits 4-7, v from bits 8-11 to bits 12-15, inclusive.  A ray tests a candidate only
// if its own sixteenth lies inside: the lists are those of a grid 16 times finer, at the memory of this one.
enum : uint32_t { SG_SINGLE = 0x80000000u, SG_PRIM_MASK = 0x0fffffffu, SG_KEY_MASK = 0xffff0000u, SG_RECT_ALL = 0xf0f0u };
struct SgEntry { uint32_t prim, key; };
// ε_tri = SG_EPS_FACTOR * 2^-23 * extent: 32 times the rounding bound C = 4 derived in DESIGN.md §11
constexpr double SG_EPS_FACTOR = 128.0;
constexpr uint32_t SG_DEFAULT_RES = 512u;

struct ShadowGrid {
    bool eligible = false;
    uint32_t R = 0;
    float light[3] = {0, 0, 0};
    // entries[0 .. nNear): the near list, which every ray tests; then the cells' lists: cell c = (face * R + iv) * R + iu holds
    // entries[cellStart[c] .. cellStart[c + 1]), keys ascending
    std::vector<uint32_t> cellStart;      // 6 R^2 + 1
    std::vector<SgEntry> entries;
    uint32_t nNear = 0, longest = 0;
    double eps = 0, buildSeconds = 0;
    size_t bytes() const { return cellStart.size() * sizeof(uint32_t) + entries.size() * sizeof(SgEntry); }
};

// tris: 12 floats per ordered primitive, the triangle records {p0, .} {p1, .} {p2, .} (DevScene::tris); single: per primitive, its
// leaf is that one triangle with the vertices' min / max as its box (null: none is).  bmin / bmax: the scene's world bound.
// R is halved until the lists hold at most maxEntries entries.  maxCandidates > 0: the cost model below — a grid whose near list plus
// mean cell list is longer comes back not eligible, decided before the lists are filled and sorted (the near list alone: before they are counted).
void BuildShadowGrid(const float *tris, const uint8_t *single, uint32_t nPrims, const float light[3], const float bmin[3],
                     const float bmax[3], uint32_t R, size_t maxEntries, double maxCandidates, ShadowGrid *out);

// The image of a grid that k_shadow_grid reads: the lists with their triangles in list order, so that a ray's candidates arrive
// with the words that name them instead of being gathered from all over the triangle array.
//
// blocks: one 128-byte block per cell, at cell * 128 — eight 16-byte words, of which the kernel reads the first seven:
//   W0 {entry count, record index of the cell's third entry, prim[0], key[0]}
//   W1 {p0 of triangle 0, prim[1]}    W2 {p1 of triangle 0, key[1]}    W3 {p2 of triangle 0, key[2]}
//   W4 {p0 of triangle 1, 0}          W5 {p1 of triangle 1, 0}         W6 {p2 of triangle 1, 0}         W7 {0, 0, 0, 0}
// (prim[k], key[k]: the two words of the list's entry k, as SgEntry holds them; words of entries the list does not have are 0.)
// The first two candidates of a list are tested from the block alone, and key[2] tells a ray whether the third concerns it.
//
// records: 48 bytes per entry, {p0, prim} {p1, key} {p2, key of the next entry of the same run (0 behind the last)}: the near list
// as one run at record 0, then per cell, in cell order, the run of its entries from the third on; SG_PAD_RECORDS records of zeros
// behind the last, so that no read of a record the kernel can form leaves the buffer.
// The vertex floats are those of the triangle records, bit for bit.
enum : uint32_t { SG_BLOCK_WORDS = 32u, SG_BLOCK_SLOTS = 2u, SG_RECORD_WORDS = 12u, SG_PAD_RECORDS = 1u };
struct ShadowGridImage {
    uint32_t R = 0, nNear = 0;
    size_t nRecords = 0;                 // near list + overflow runs, without the padding
    std::vector<uint32_t> blocks;        // faces * R^2 * SG_BLOCK_WORDS (faces * R^2 = the grid's cellStart.size() - 1)
    std::vector<uint32_t> records;       // (nRecords + SG_PAD_RECORDS) * SG_RECORD_WORDS
    double packSeconds = 0;
    size_t bytes() const { return (blocks.size() + records.size()) * sizeof(uint32_t); }
};
// the bytes PackShadowGrid's image of g takes, without forming it
size_t ShadowGridImageBytes(const ShadowGrid &g);
// tris: the triangle records BuildShadowGrid was given
void PackShadowGrid(const ShadowGrid &g, const float *tris, ShadowGridImage *out);

// HPRT_SHADOW_GRID: 0 no grid (A/B runs), 1 a grid for every scene that can have one, unset (-1) only where it is expected to
// be cheaper than the walk (SG_MAX_CANDIDATES); HPRT_SHADOW_GRID_RES: cells per face side.  Read per scene.
int ShadowGridModeFromEnv();
// A ray tests the near list and, at most, its cell's list; a candidate costs four memory requests, the any-hit walk about 55 per ray
// (DESIGN.md §4).  A grid whose near list plus mean cell list is longer than this is not expected to beat the walk — a light wrapped
// closely in fine geometry, or a mesh with many degenerate triangles, which all go to the near list — and is dropped.
constexpr double SG_MAX_CANDIDATES = 14.0;
uint32_t ShadowGridResFromEnv();

}  // namespace hprt
