// hprt host side — builder for Accelerator "bvhold", the stock pbrt-v3 BVH the fork keeps as BVHAccelOld
// (accelerators/bvhOld.cpp:185-227): recursiveBuild (:238-404) for the split methods sah, middle and equal, HLBVHBuild /
// emitLBVH / buildUpperSAH (:406-640) for hlbvh, flattenBVHTree (:642-660).  The result is the project's BvhTree: the 32-byte
// nodes of bvh_builder.h (an interior node's count is 0, as LinearBVHNodeOld::nPrimitives is) and primOrder, the reference's
// orderedPrims.  std::partition and std::nth_element are called themselves, over pointers as the reference calls them, so
// that with the same libstdc++ they permute primitiveInfo as the reference's do.
//
// Two places where the reference does not fix the bytes, and what is fixed here:
//  * recursiveBuild's two recursive calls are the arguments of one InitInterior call (:396-400), whose order of evaluation
//    C++ leaves open.  g++ evaluates the second first; so does this builder, explicitly: a node's second child takes its
//    leaves' offsets before its first child does.  (Only leaf offsets and primOrder see it; no walk does.)
//  * HLBVHBuild's treelets take their leaves' offsets with fetch_add from parallel tasks (:452-464, :488).  Here a treelet's
//    leaves take their offsets in treelet order, so primOrder is the sorted Morton array — what the reference gives on one
//    thread.  The tree does not depend on a thread count.
#pragma once
#include <cstdint>
#include <string>
#include <vector>
#include "bvh_builder.h"

namespace hprt {

enum { BVHOLD_SAH = 0, BVHOLD_HLBVH = 1, BVHOLD_MIDDLE = 2, BVHOLD_EQUAL = 3 };     // == HPRT_BVHOLD_*
struct BvhOldParams {              // CreateBVHAcceleratorOld, accelerators/bvhOld.cpp:742-762
    int32_t splitMethod = BVHOLD_SAH, maxNodePrims = 4;
};
constexpr uint32_t kBvhOldMaxLeaf = 65536;       // CHECK_LT(node->nPrimitives, 65536), :648

// "" and the tree, or why the reference's build is undefined for this input (the tree is then empty): the CHECK_NE of :566
// (the treelet roots' centroids coincide on the widest axis), the CHECK_GE / CHECK_LT of :331-332 and :585-586 (a centroid
// outside the 12 SAH buckets: bounds that are not finite, or whose sum overflows) and a leaf of kBvhOldMaxLeaf primitives or more.
// n == 0 gives the empty tree (:191).  bmin / bmax: 3 floats per primitive, creation order.
std::string BuildBvhOld(size_t n, const float *bmin, const float *bmax, const BvhOldParams &params, BvhTree *out);

// ---- the steps of the HLBVH form, shared with the device build (device/hlbvh_build.hip) ----
namespace hlbvh {

struct MortonPrim { uint32_t code, index; };     // MortonPrimitiveOld, as the sort moves it
static_assert(sizeof(MortonPrim) == 8, "MortonPrim is 8 bytes");
constexpr uint32_t kTreeletMask = 0x3ffc0000u;   // the top 12 of the 30 bits (:437)
constexpr int kFirstBit = 29 - 12;               // emitLBVH starts here (:457)
constexpr uint32_t kMaxTreelets = 4096;

// A treelet: mortonPrims[start, start + count); its nodes are nodes[nodeBase, nodeBase + nNodes) of a shared array, in
// preorder, interior offsets relative to nodeBase, leaf offsets the sorted position of the leaf's first primitive
struct Treelet { uint32_t start, count, nodeBase, nNodes; };

// The bounds of the centroids (.5f * pMin + .5f * pMax, :54): lo[3], hi[3]
void CentroidBounds(size_t n, const float *bmin, const float *bmax, float lo[3], float hi[3]);
// Bounds3::Offset (geometry.h:972-978), * 1024, truncation, EncodeMorton3 (:109-139).  The truncation is the device's, spelled
// out: past 1024 gives 1024, a NaN or a negative value 0 (finite bounds whose extent overflows reach both); never undefined.
uint32_t MortonCode(const float cen[3], const float lo[3], const float hi[3]);
// A stable sort by the 30-bit code (std::stable_sort): the array the reference's own LSD radix sort (:141-182) gives
void SortMorton(std::vector<MortonPrim> *v);
// The intervals of equal top 12 bits (:433-449); nodeBase = 2 * start (a treelet of k primitives has at most 2 k - 1 nodes)
void FindTreelets(const MortonPrim *sorted, size_t n, std::vector<Treelet> *out);
// emitLBVH (:476-538) for one treelet, iteratively: writes nodes[t->nodeBase ...] and t->nNodes.  "" or the refusal
// (a leaf of kBvhOldMaxLeaf primitives or more).
std::string EmitTreelet(const MortonPrim *sorted, Treelet *t, int maxPrimsInNode, const float *bmin, const float *bmax, BvhNode *nodes);
// buildUpperSAH (:540-640) over the treelets' roots and the final depth-first array: interior offsets gain the treelet's
// place, primOrder is the sorted array's indices.  "" or the refusal of :566.
std::string Assemble(const MortonPrim *sorted, size_t n, const std::vector<Treelet> &treelets, const BvhNode *nodes, BvhTree *out);

}  // namespace hlbvh
}  // namespace hprt
