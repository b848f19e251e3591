// hprt — the node array every GenericBSP tree of the fork shares (accelerators/genericBSP.h): 8-byte nodes {a, b} over M split
// directions, off = 32 - clz(M) flag bits, mask = (1 << off) - 1:
//   a: interior split (float bits) | leaf onePrimitive (one primitive) | leaf primitiveIndicesOffset (more than one) | 0 (empty leaf)
//   b: interior direction | aboveChild << off;  leaf M | nPrimitives << off.  A node is a leaf iff (b & mask) == M.
// The kd-tree's KdAccelNode is the case M = 3 (off = 2, mask = 3).  Header-only: the builders' own checks call it.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace hprt {

struct BspNode { uint32_t a, b; };
static_assert(sizeof(BspNode) == 8, "BspNode must be 8 bytes");

// Structural check of a tree handed to the device: child offsets, leaf index ranges, primitive numbers, depth.  Returns an
// empty string when the tree is well-formed, else what is wrong; *depthOut: the interior levels of the deepest path.
inline const char *CheckBspNodes(const std::vector<BspNode> &nodes, const std::vector<uint32_t> &primIndices, uint32_t nPrims, uint32_t M, uint32_t off,
                                 uint32_t mask, uint32_t *depthOut) {
    const size_t n = nodes.size();
    if (n == 0) return "the tree has no nodes";
    if (n >= (1ull << (32 - off))) return "too many nodes for the child offset field";
    // children always follow their parent (below child = next node, above child further on), so depths fill back to front
    std::vector<uint32_t> depth(n, 0);
    for (size_t k = n; k-- > 0;) {
        const BspNode &nd = nodes[k];
        if ((nd.b & mask) == M) {
            const uint32_t np = nd.b >> off;
            if (np == 1) { if (nd.a >= nPrims) return "a one-primitive leaf names a primitive that does not exist"; }
            else if (np > 1) {
                if ((uint64_t)nd.a + np > primIndices.size()) return "a leaf's primitive range runs past primitiveIndices";
                for (uint32_t i = 0; i < np; ++i)
                    if (primIndices[nd.a + i] >= nPrims) return "primitiveIndices names a primitive that does not exist";
            }
        } else {
            if ((nd.b & mask) > M) return "an interior node's direction is out of range";
            const uint32_t above = nd.b >> off;
            if (k + 1 >= n) return "an interior node has no below child";
            if (above <= k + 1 || above >= n) return "an interior node's above child is out of range";
            depth[k] = 1 + std::max(depth[k + 1], depth[above]);
        }
    }
    if (depthOut) *depthOut = depth[0];
    return "";
}

}  // namespace hprt
