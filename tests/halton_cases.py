"""What tests/test_halton_host.py and tests/test_gpu_halton.py share: the Halton indices at which a radical inverse can go wrong, per
dimension, the sampler layouts, a plain Python model of HaltonSampler::SampleDimension, and the sample numbers that put a Halton
index on either side of 2^32 or far above it."""
import numpy as np

N_DIMS = 1000                                   # PrimeTableSize (core/lowdiscrepancy.h:52)
LDS_DIMS = 64                                   # HPRT_HALTON_LDS_DIMS: k_shade reads dimensions below it from the LDS copy
# sample bounds (sx0, sy0, sx1, sy1): stride 1; 32 * 27; 128 * 243 (both at kMaxResolution); the killeroo frame's 128 * 243
LAYOUTS = {"1x1": (0, 0, 1, 1), "17x23": (0, 0, 17, 23), "128x128": (0, 0, 128, 128), "700x700": (0, 0, 700, 700)}
ONE_MINUS_EPS = np.float32(np.nextafter(np.float32(1), np.float32(0)))


def primes():
    sieve = np.ones(8000, bool)
    sieve[:2] = False
    for i in range(2, 90):
        if sieve[i]:
            sieve[i * i::i] = False
    p = np.flatnonzero(sieve)[:N_DIMS]
    assert p.size == N_DIMS and p[-1] == 7919
    return [int(x) for x in p]


def edge_indices(b):
    """The hand-picked indices of base b: around the first digits, around every power of b below 2^63, around 2^31, 2^32 and at
    2^63 - 1, and around the largest 32-bit multiple of b (where the 32-bit quotient estimate and its one-compare repair, and the
    truncation of the reversed digits to 32 bits, are closest to their limits)."""
    out = [0, 1, b - 1, b, b + 1]
    p = b
    while p < 2 ** 63:
        out += [p - 1, p, p + 1]
        p *= b
    out += [2 ** 31 - 1, 2 ** 31 + 1] + [2 ** 32 + k for k in range(-2, 3)] + [2 ** 63 - 1]
    m = (2 ** 32 - 1) // b * b
    out += [m - 1, m, m + 1, m + b - 1]
    return [v for v in out if 0 <= v < 2 ** 63]


def dimension_indices(b, rng, n_random=400):
    """uint64 indices of base b: edge_indices plus n_random 32-bit values, n_random 32-bit multiples of b and n_random values of a random
    bit length up to 63."""
    edges = np.array(edge_indices(b), np.uint64)
    r32 = rng.integers(0, 2 ** 32, n_random, dtype=np.uint64)
    mult = rng.integers(0, (2 ** 32 - 1) // b + 1, n_random, dtype=np.uint64) * np.uint64(b)
    bits = rng.integers(1, 64, n_random).astype(np.uint64)
    wide = (rng.integers(0, 2 ** 63, n_random, dtype=np.uint64) | np.uint64(2 ** 62)) >> (np.uint64(63) - bits)      # bit length exactly `bits`
    return np.concatenate([edges, r32, mult, wide])


def pairs(dims, seed, n_random=400):
    """(index uint64[], dim int32[]) over `dims`: dimension_indices of each dimension's base, seeded per dimension"""
    pr = primes()
    idx, dim = [], []
    for d in dims:
        v = dimension_indices(pr[d], np.random.default_rng([seed, d]), n_random)
        idx.append(v)
        dim.append(np.full(v.size, d, np.int32))
    return np.concatenate(idx), np.concatenate(dim)


def layout(bounds):
    """(baseScales, baseExponents) of HaltonSampler's constructor (samplers/halton.cpp:73-85)"""
    scales, exps = [], []
    for base, res in ((2, bounds[2] - bounds[0]), (3, bounds[3] - bounds[1])):
        scale, exp = 1, 0
        while scale < min(res, 128):
            scale *= base
            exp += 1
        scales.append(scale)
        exps.append(exp)
    return scales, exps


def model_sample_dimension(bounds, center, index, dim, perms, prime_sums, pr):
    """HaltonSampler::SampleDimension (samplers/halton.cpp:119-127) over RadicalInverse / ScrambledRadicalInverse
    (core/lowdiscrepancy.cpp:389-436): Python integers for the digit loop and the wrap modulo 2^64, np.float32 for each float
    operation in the reference's order."""
    f32 = np.float32
    scales, exps = layout(bounds)
    if center and dim in (0, 1):
        return f32(0.5)
    if dim == 0:
        a = index >> exps[0]
        rev = int(format(a, "064b")[::-1], 2)
        return f32(float(rev) * 2.0 ** -64)                      # uint64 -> double (one rounding), exact scale, double -> float
    a = index // scales[1] if dim == 1 else index
    base = pr[dim]
    inv_base = f32(1) / f32(base)
    perm = perms[prime_sums[dim]:prime_sums[dim] + base] if dim > 1 else None
    rd, inv_base_n = 0, f32(1)
    while a:
        nxt = a // base
        digit = a - nxt * base
        rd = (rd * base + (int(perm[digit]) if dim > 1 else digit)) & (2 ** 64 - 1)
        inv_base_n = inv_base_n * inv_base
        a = nxt
    rdf = f32(np.uint64(rd))
    if dim == 1:
        v = rdf * inv_base_n
    else:
        v = inv_base_n * (rdf + inv_base * f32(int(perm[0])) / (f32(1) - inv_base))
    return min(v, ONE_MINUS_EPS)


def straddling_samples(rng, n, stride):
    """n sample numbers for a sampler of that stride: half in the four whose Halton index crosses 2^32 depending on the pixel's offset
    (2^32 / stride = 138,084.35 for the 700 x 700 frame's 31,104), half about 2^e / stride with e uniform in [32, 62]."""
    k = 2 ** 32 // stride
    near = rng.integers(k - 1, k + 3, n // 2)
    e = rng.uniform(32, 62, n - n // 2)
    far = np.floor(2.0 ** e / stride).astype(np.int64)
    return np.concatenate([near, far]).astype(np.int64)
