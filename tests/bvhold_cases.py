"""What the bvhold tests share (tests/test_bvhold_host.py on the CPU, tests/test_gpu_bvhold.py on the GPU): the box sets the
HLBVH form is held to, as (bmin, bmax, maxnodeprims), a numpy statement of the Morton codes, and the numbering that makes hits
through two trees of one scene comparable."""
import numpy as np

SORT_TILE = 2048          # keys per workgroup and pass of the device sort (device/hlbvh_build.hip: kTile)


def _boxes(c, h):
    c = np.asarray(c, np.float32); h = np.asarray(h, np.float32)
    return (c - h).astype(np.float32), (c + h).astype(np.float32)


def random_boxes(n, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-10, 10, (n, 3)).astype(np.float32)
    h = rng.uniform(0.01, 0.5, (n, 3)).astype(np.float32)
    return _boxes(c, h)


def edge_shapes():
    """name -> (bmin, bmax, maxnodeprims): the HLBVH edge shapes.  Centres and half sizes of the made-up sets are small multiples
    of 1/8, so that .5f * pMin + .5f * pMax is the centre exactly."""
    rng = np.random.default_rng(1234)
    shapes = {}
    for n in (1, 2, 3, 4, 5, 64, 65, 257, 4097):          # 1, 2, 3 with maxnodeprims 4: the root is a leaf (the strict <)
        shapes["n%d" % n] = random_boxes(n, 100 + n) + (4,)
    n = 300                                               # all centroids equal: one leaf of n primitives
    shapes["all_equal"] = _boxes(np.tile([[1.0, 2.0, 3.0]], (n, 1)), rng.integers(1, 40, (n, 3)) / 8.0) + (4,)
    c = (rng.integers(0, 200, (500, 3)) / 8.0).astype(np.float32); c[:, 2] = 5.0      # zero extent on z
    shapes["flat_axis"] = _boxes(c, rng.integers(1, 9, (500, 3)) / 8.0) + (4,)
    c = rng.integers(0, 4, (5000, 3)).astype(np.float32)                              # a 4x4x4 lattice: bit-exhausted leaves of ~78 primitives
    shapes["lattice"] = _boxes(c, rng.integers(1, 9, (5000, 3)) / 8.0) + (4,)
    c = (rng.integers(0, 1025, (600, 3))).astype(np.float32); c[:7] = 1024.0; c[7:9, 0] = 1024.0; c[9] = 0.0      # offsets of exactly 1.0: the x == 1024 decrement
    shapes["offset_one"] = _boxes(c, rng.integers(1, 9, (600, 3)) / 8.0) + (4,)
    shapes["n70001"] = random_boxes(70001, 7) + (4,)
    # a treelet of two clusters of 140 primitives each: maxnodeprims 255 splits it, anything from 281 on would not
    c = np.zeros((281, 3), np.float32); c[:140] = [0.0, 0.0, 0.0]; c[140:280] = [1.0, 0.0, 0.0]; c[280] = [1024.0, 1024.0, 1024.0]
    shapes["clamp"] = _boxes(c, rng.integers(1, 9, (281, 3)) / 8.0) + (300,)
    return shapes


def sort_shapes():
    """name -> (bmin, bmax, maxnodeprims): sets that stress the device sort (the GPU test adds them to edge_shapes())"""
    rng = np.random.default_rng(4321)
    shapes = {}
    for n in (SORT_TILE - 1, SORT_TILE, SORT_TILE + 1, 4 * SORT_TILE - 1, 4 * SORT_TILE, 4 * SORT_TILE + 1):
        shapes["tile%d" % n] = random_boxes(n, 200 + n) + (4,)
    # codes that differ in the top digit only (multiples of 256 of 1024 per axis) and in the bottom digit only (0..3 of 1024); the
    # one box at 1024 that sets the extent has all bits set
    for name, step in (("top_digit", 256), ("bottom_digit", 1)):
        c = (rng.integers(0, 4, (3000, 3)) * step).astype(np.float32); c[0] = 1024.0
        shapes[name] = _boxes(c, rng.integers(1, 9, (3000, 3)) / 8.0) + (4,)
    # 8,192 equal codes across workgroup boundaries: the order of the equal keys is the sort's stability
    shapes["equal_codes"] = _boxes(np.tile([[3.0, 3.0, 3.0]], (8192, 1)), rng.integers(1, 40, (8192, 3)) / 8.0) + (4,)
    return shapes


def huge_extent(flat=False):
    """(bmin, bmax): finite boxes whose centroid extent overflows on x (hi - lo is inf there, and the largest c - lo too): the
    Offset is 0 or NaN, and the build must form its codes without an undefined float-to-integer conversion.  flat: no extent on
    y and z, so that every code is 0 and the tree is one leaf (no upper SAH, whose (pMin + pMax) would overflow)"""
    rng = np.random.default_rng(77)
    c = rng.uniform(-1, 1, (200, 3)).astype(np.float32)
    c[:, 0] *= np.float32(3e38)
    c[0, 0], c[1, 0] = np.float32(-3e38), np.float32(3e38)
    if flat:
        c[:, 1:] = 0
    return c.copy(), c.copy()


def morton_codes(bmin, bmax):
    """the 30-bit codes of HLBVHBuild in float32 numpy: centroid, Bounds3::Offset, * 1024, truncation, the 1024 decrement, bit spreading"""
    bmin = np.asarray(bmin, np.float32); bmax = np.asarray(bmax, np.float32)
    c = (np.float32(.5) * bmin + np.float32(.5) * bmax).astype(np.float32)
    lo, hi = c.min(0), c.max(0)
    o = (c - lo).astype(np.float32)
    ext = (hi - lo).astype(np.float32)
    for k in range(3):
        if hi[k] > lo[k]:
            o[:, k] = (o[:, k] / ext[k]).astype(np.float32)
    q = (o * np.float32(1024)).astype(np.float32).astype(np.uint32)
    q[q == 1024] = 1023

    def spread(x):
        x = (x | (x << 16)) & 0x30000ff
        x = (x | (x << 8)) & 0x300f00f
        x = (x | (x << 4)) & 0x30c30c3
        x = (x | (x << 2)) & 0x9249249
        return x
    return (spread(q[:, 2]) << 2) | (spread(q[:, 1]) << 1) | spread(q[:, 0])


def creation_ids(prim, orders):
    """a hit's ordered primitive over all aggregates (top level first, then object 0, 1, ...; -1: none) as the primitive's
    creation number in the same layout: comparable between two trees of one scene.  orders: [top order, object 0's, ...]"""
    flat, base = [], 0
    for o in orders:
        flat.append(np.asarray(o, np.int64) + base)
        base += len(o)
    flat = np.concatenate(flat) if flat else np.zeros(0, np.int64)
    prim = np.asarray(prim, np.int64)
    out = np.full(prim.shape, -1, np.int64)
    out[prim >= 0] = flat[prim[prim >= 0]]
    return out
