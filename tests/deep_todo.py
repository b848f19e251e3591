"""A staircase scene whose rays hold a known number of todo entries, for the walks' todo lists past their LDS entries
(tests/test_deep_todo_host.py, tests/test_gpu_deep_todo.py): the generator, its five tree encodings, the ray families and the checks
on the restatements alone.

The staircase of L levels (L <= 64) has the split positions s_k = k along x, k = 0 .. L-1.  Interior node k of the chain sends its
+x side to the next chain node and its -x side to a sibling subtree: one split over two one-triangle leaves (on y, or along
(0, 1, 1) / sqrt 2 where an encoding wants an oblique node), so that the popped tMin and tMax decide which of the two leaves is
fetched.  The last chain node has two leaves: a one-triangle leaf below and a two-triangle leaf (primitiveIndices) above.  A
sibling subtree there would make the tree L + 1 levels deep while no ray could hold more than L entries: the deepest path must
push at every level for a ray to reach the capacity of a tree that attach still accepts.

Every triangle lies in a plane x = const of its own, strictly inside its slab: the triangles are mutually parallel and no two are
at the same t for a ray with d.x != 0, so there are no ties and the closest hit does not depend on the visiting order.

A ray of the deep family starts at x > s_{L-1} with d.x < 0: every chain node's plane lies ahead of it, nearest last, so the walk
pushes one entry per level before it reaches its first leaf and holds exactly j entries at level j.  A finite tMax that ends
between the planes L-m and L-m-1 stops the pushes at m entries.  The sibling subtrees push only after a pop, so they never raise
the count.  The mirrored family (d.x > 0 from x < s_0, both ends in one open quadrant of y, z so that no sibling split is crossed)
pops what it pushes at once and never holds more than one entry: the control."""
import os

import numpy as np

LEVELS = (1, 7, 8, 9, 10, 16, 17, 33, 63, 64)      # the levels a finite tMax stops at: each walk's LDS count +-1 (k_trace's 7, 10, 16 too), and the capacity
CAPACITY = 64
RBSP_M, RBSPKD_M = 7, 9
RBSPKD_OBLIQUE = 5                                # (0, 1, 1) / sqrt 2 in getDirections(9)
TREES = ("kdtree", "rbsp", "rbspkd", "bsppaper", "bsppaperkd")


def _f2u(x):
    return int(np.float32(x).view(np.uint32))


class Staircase:
    """L levels: tris [n, 3, 3] float32 in creation order (n = 2 L + 1), bounds (6 floats), and with sphere=True one sphere (primitive
    n) in the last slab, tested in the last leaf."""

    def __init__(self, L, seed=0, sphere=False):
        assert 1 <= L
        self.L, self.sphere = L, sphere
        rng = np.random.default_rng(seed)
        n = 2 * L + 1
        x = np.zeros(n, np.float32)
        lowq = np.zeros(n, bool)                  # the triangle lies in y < 0, z < 0 (else in y > 0, z > 0 where it shares a sibling subtree)
        for k in range(L - 1):
            x[2 * k], x[2 * k + 1] = k - 0.6, k - 0.4
            lowq[2 * k] = True
        x[2 * L - 2] = L - 1 - 0.5
        x[2 * L - 1], x[2 * L] = L - 1 + 0.4, L - 1 + 0.6
        lowq[2 * L - 2] = True
        y0 = np.where(lowq, rng.uniform(-0.95, -0.65, n), rng.uniform(0.15, 0.45, n))
        z0 = np.where(lowq, rng.uniform(-0.95, -0.65, n), rng.uniform(0.15, 0.45, n))
        w = 0.5
        T = np.zeros((n, 3, 3), np.float32)
        T[:, :, 0] = x[:, None]
        T[:, 0, 1], T[:, 0, 2] = y0, z0
        T[:, 1, 1], T[:, 1, 2] = y0 + w, z0
        T[:, 2, 1], T[:, 2, 2] = y0, z0 + w
        self.tris = T
        self.n_prims = n + (1 if sphere else 0)
        self.sphere_center, self.sphere_radius = (L - 1 + 0.5, 0.0, 0.0), 0.08
        lo, hi = T.reshape(-1, 3).min(0), T.reshape(-1, 3).max(0)
        if sphere:
            c, r = np.array(self.sphere_center, np.float32), np.float32(self.sphere_radius)
            lo, hi = np.minimum(lo, c - r), np.maximum(hi, c + r)
        self.bounds = np.concatenate([lo, hi]).astype(np.float32)

    # ---- the model: the triangles as a .pbrt mesh, parsed and baked, so that model, oracle and restatements load one file ----
    def bake(self, hprt, directory):
        """path of the baked scene; the camera looks down -x from beyond the last level, so narrowly that a camera ray passes most of the
        levels before it leaves the bounds (700 x 700 pixels: tree_walk_checks.check_counting_render's crop is 48 x 40 of them)"""
        L = self.L
        P = self.tris.reshape(-1, 3)
        text = ("LookAt %r 0.05 0.1  0 0 0  0 0 1\n" % float(L + 2.0) +
                'Camera "perspective" "float fov" [12]\nFilm "image" "integer xresolution" [700] "integer yresolution" [700]\n'
                'Sampler "halton" "integer pixelsamples" [2]\nIntegrator "path" "integer maxdepth" [3]\nAccelerator "bvh"\nWorldBegin\n'
                'LightSource "point" "point from" [%r 0 0] "color I" [400 400 400]\n' % float(L + 1.0) +
                'Shape "trianglemesh" "integer indices" [' + " ".join(map(str, range(P.shape[0]))) + '] "point P" [' +
                " ".join(repr(float(v)) for v in P.ravel()) + "]\n")
        if self.sphere:
            text += 'AttributeBegin Translate %r %r %r Shape "sphere" "float radius" [%r] AttributeEnd\n' % (self.sphere_center + (self.sphere_radius,))
        text += "WorldEnd\n"
        stem = os.path.join(str(directory), "staircase%d%s" % (L, "s" if self.sphere else ""))
        with open(stem + ".pbrt", "w") as f:
            f.write(text)
        m = hprt.Model.parse(stem + ".pbrt")
        m.save(stem + ".hprt")
        return stem + ".hprt"

    # ---- the five encodings of one tree ----
    def _layout(self):
        """the nodes in order: (kind, ...) with ("x", k, above) a chain node, ("y", k, above) a sibling split, ("leaf", prims)"""
        L, out = self.L, []
        for k in range(L - 1):
            out += [("x", k, 4 * k + 4), ("y", k, 4 * k + 3), ("leaf", [2 * k]), ("leaf", [2 * k + 1])]
        last = [2 * L - 1, 2 * L] + ([2 * L + 1] if self.sphere else [])
        out += [("x", L - 1, 4 * (L - 1) + 2), ("leaf", [2 * L - 2]), ("leaf", last)]
        return out

    def _encode(self, words, shift, leaf_tag, interior):
        """nodes [n, words] uint32 and primitiveIndices; interior(kind, k) -> (flag bits, axis or None)"""
        lay = self._layout()
        nodes = np.zeros((len(lay), words), np.uint32)
        idx = []
        for i, nd in enumerate(lay):
            if nd[0] == "leaf":
                prims = nd[1]
                nodes[i, 1] = leaf_tag | (len(prims) << shift)
                if len(prims) == 1:
                    nodes[i, 0] = prims[0]
                else:
                    nodes[i, 0] = len(idx)
                    idx += prims
            else:
                kind, k, above = nd
                tag, axis = interior(kind, k)
                nodes[i, 0] = _f2u(float(k) if kind == "x" else 0.0)
                nodes[i, 1] = tag | (above << shift)
                if axis is not None:
                    nodes[i, 2:5] = np.array(axis, np.float32).view(np.uint32)
        return nodes, np.array(idx, np.uint32)

    def kdtree(self):
        return self._encode(2, 2, 3, lambda kind, k: (0 if kind == "x" else 1, None))

    def rbsp(self):
        """direction 0 and direction 1 of getDirections(7): every node takes the dot-product step"""
        return self._encode(2, 3, RBSP_M, lambda kind, k: (0 if kind == "x" else 1, None))

    def rbspkd(self):
        """The chain is direction 0, which the rbspkd walk takes as a kd node (every direction below 3 is one: no dot node can split
        on x alone).  The dot-product step crosses the seam in the sibling subtrees instead: at odd levels they split along
        (0, 1, 1) / sqrt 2 of getDirections(9), at even levels on y, and a sibling's push at level j lands on entry j."""
        return self._encode(2, 4, RBSPKD_M, lambda kind, k: (0 if kind == "x" else (RBSPKD_OBLIQUE if k % 2 else 1), None))

    def bsppaper(self):
        return self._encode(5, 1, 1, lambda kind, k: (0, (1, 0, 0) if kind == "x" else (0, 1, 0)))

    def bsppaperkd(self):
        """kd and plane nodes alternate level by level, along the chain and (the other way round) in the sibling subtrees"""
        def interior(kind, k):
            kd = (k % 2 == 0) == (kind == "x")
            if kd:
                return (0 if kind == "x" else 1), None
            return 4, ((1, 0, 0) if kind == "x" else (0, 1, 0))
        return self._encode(5, 3, 3, interior)

    def arrays(self, tree):
        return getattr(self, tree)()

    def handle(self, hprt, tree):
        """the library's handle of this tree (hprt_debug_<tree>_from_arrays)"""
        nodes, idx = self.arrays(tree)
        cls = {"kdtree": hprt.KdTree, "rbsp": hprt.Rbsp, "rbspkd": hprt.RbspKd, "bsppaper": hprt.BspPaper, "bsppaperkd": hprt.BspPaperKd}[tree]
        extra = {"rbsp": (RBSP_M,), "rbspkd": (RBSPKD_M,)}.get(tree, ())
        return cls.from_arrays(nodes, idx, self.n_prims, self.bounds, *extra)

    def reference(self, tree, path):
        """the restatement of `tree` over the baked scene at `path`, walking these arrays"""
        import bsppaperkd_ref
        import tree_ref
        nodes, idx = self.arrays(tree)
        if tree == "kdtree":
            ref = tree_ref.KdScene(path)
        elif tree == "rbsp":
            ref = tree_ref.RbspScene(path, RBSP_M, build=False)
        elif tree == "rbspkd":
            ref = tree_ref.RbspKdScene(path, RBSPKD_M, build=False)
        elif tree == "bsppaper":
            ref = tree_ref.BspScene(path, build=False)
        else:
            ref = bsppaperkd_ref.BspKdScene(path, build=False)
        ref.set_tree(nodes, idx)
        return ref

    # ---- the ray families ----
    def levels(self):
        """the levels of LEVELS this staircase has (a finite tMax cannot stop deeper than L)"""
        return tuple(sorted({min(m, self.L) for m in LEVELS}))

    def deep_rays(self, n, seed=1):
        """(o, d, tmax, level): ray i is meant to hold `level[i]` entries at most.  Even i: tMax = inf (level L).  Odd i: a finite
        tMax that stops the descent at LEVELS[(i % 64) // 2 % 10], so that each of the ten levels is the aim of 3 or 4 of every 64
        consecutive rays and every wave mixes lanes that stay in LDS with lanes deep in HBM.  (i // 64) % 8 = 1 .. 4: d.y = +0,
        d.y = -0, d.z = -0, d.y = +0 and d.z = -0."""
        L = self.L
        rng = np.random.default_rng(seed)
        i = np.arange(n)
        o = np.stack([L - 1 + 0.7 + rng.uniform(0, 0.2, n), rng.uniform(-0.8, 0.8, n), rng.uniform(-0.8, 0.8, n)], 1).astype(np.float32)
        end = np.stack([np.full(n, -1.0), rng.uniform(-0.8, 0.8, n), rng.uniform(-0.8, 0.8, n)], 1)
        d = ((end - o) * rng.uniform(0.5, 2.0, n)[:, None]).astype(np.float32)
        z = (i // 64) % 8
        d[:, 1] = np.where((z == 1) | (z == 4), np.float32(0.0), np.where(z == 2, np.float32(-0.0), d[:, 1]))
        d[:, 2] = np.where((z == 3) | (z == 4), np.float32(-0.0), d[:, 2])
        level = np.where(i % 2 == 0, L, np.minimum(np.array(LEVELS)[(i % 64) // 2 % len(LEVELS)], L))
        # a finite tMax ends half a slab beyond the last plane it is to cross, s_{L - level}
        stop_x = (L - level) - 0.5
        tm = np.where(i % 2 == 0, np.inf, (stop_x - o[:, 0].astype(np.float64)) / d[:, 0].astype(np.float64)).astype(np.float32)
        return o, d, tm, level

    def control_rays(self, n, seed=2):
        """the mirrored family: d.x > 0 from x < s_0, both ends in one open quadrant of y, z (no sibling split is crossed)"""
        L = self.L
        rng = np.random.default_rng(seed)
        sign = np.where(rng.uniform(size=n) < 0.5, -1.0, 1.0)
        o = np.stack([-0.7 - rng.uniform(0, 0.2, n), sign * rng.uniform(0.05, 0.8, n), sign * rng.uniform(0.05, 0.8, n)], 1).astype(np.float32)
        end = np.stack([np.full(n, float(L)), sign * rng.uniform(0.05, 0.8, n), sign * rng.uniform(0.05, 0.8, n)], 1)
        d = ((end - o) * rng.uniform(0.5, 2.0, n)[:, None]).astype(np.float32)
        d[::8, 1] = 0.0
        d[4::8, 2] = -0.0
        tm = np.where(np.arange(n) % 2 == 0, np.inf, rng.uniform(0.1, 1.2, n)).astype(np.float32)
        return o, d, tm


def check_no_ties(stairs):
    """the construction that makes the closest hit independent of the accelerator: every triangle in a plane x = const, no two in
    the same plane, each strictly inside its slab, and a sibling's two triangles on either side of both of its possible splits"""
    T, L = stairs.tris, stairs.L
    x = T[:, 0, 0]
    assert (T[:, :, 0] == x[:, None]).all() and np.unique(x).shape[0] == x.shape[0]
    k = np.arange(L - 1)
    for t in (2 * k, 2 * k + 1):
        assert ((x[t] > k - 1) & (x[t] < k)).all()
    assert L - 2 < x[2 * L - 2] < L - 1 and (x[2 * L - 1:] > L - 1).all()
    a, b = T[2 * k], T[2 * k + 1]
    assert (a[:, :, 1] < 0).all() and (b[:, :, 1] > 0).all()
    assert (a[:, :, 1] + a[:, :, 2] < 0).all() and (b[:, :, 1] + b[:, :, 2] > 0).all()


def check_ray_family(stairs, ref, n=4096, any_hit=False):
    """The conditions on the restatement alone, by its max_todo: every level of the list is reached — held exactly, as the deepest
    the ray went — by at least 1/32 of the rays, every ray goes exactly as deep as it was aimed, some ray reaches the capacity
    (at L = 64), and no ray of the control family exceeds 1.  Returns the deep family's max_todo."""
    o, d, tm, level = stairs.deep_rays(n)
    (ref.occluded if any_hit else ref.intersect)(o, d, tm)
    mt = ref.max_todo()
    assert mt.shape[0] == n
    assert np.array_equal(mt, level), (int((mt != level).sum()), mt[:16], level[:16])
    for m in stairs.levels():
        assert (mt == m).mean() >= 1 / 32, (m, (mt == m).mean())
    assert mt.max() == stairs.L and (stairs.L != CAPACITY or (mt == CAPACITY).any())
    oc, dc, tc = stairs.control_rays(n)
    (ref.occluded if any_hit else ref.intersect)(oc, dc, tc)
    mc = ref.max_todo()
    assert mc.max() == 1, mc.max()
    return mt


# ---- the sixth form: a binary BVH chain over the same triangles, for k_trace and (collapsed four wide) k_walk4 ----
# k_walk4's LDS counts (12 closest, 20 any) and the entry past each; 14 and 22 too, because the wide walk does not push the slot it
# goes on with and so holds one entry fewer than the binary walk on the same ray
BVH_EXTRA_LEVELS = (12, 13, 14, 20, 21, 22)
WIDE_CHAIN = 60                                   # the chain whose collapse needs exactly k_walk4's 60 entries (stack_need = chain length)
BVH_CHAIN = 63                                    # interior levels: a BVH of 64 node levels is the deepest hprt_scene_create takes


class BvhChain:
    """The staircase of N levels as a binary BVH chain given through SceneDesc: interior node k (split axis 0, index k) has the next
    interior node as its first child and the leaf of slab k as its second (the two triangles 2k, 2k+1).  The last one has the leaf of
    the triangles 2N-2, 2N-1 (one in either quadrant, so its box spans both) as its first child and the last triangle alone as its
    second: a ray through that triangle's box then meets all three leaf boxes of the last wide record, and holds stack_need entries.  Every box is the exact union of its triangles' bounds.

    BVHAccel::Intersect pushes the far child: with split axis 0 a ray with d.x < 0 pushes the chain and visits the leaf, and never
    holds more than two entries.  The deep family is therefore the mirrored one: d.x > 0 from x < s_0, which pushes leaf k and goes
    on to chain node k + 1 for as long as it enters the chain's boxes, and holds exactly j entries at level j.  A ray stays inside
    the y, z extent of the innermost box (|y|, |z| <= 0.6), so it enters chain node k's box through its face x = k - 0.6, and a
    finite tMax that ends between two such faces stops the pushes at a known level.  N = 63 is the binary limit (a chain of N
    interior levels is N + 1 node levels deep, and 64 are accepted), so the deepest ray holds 63 entries, not 64."""

    def __init__(self, N=BVH_CHAIN, seed=0):
        self.N, self.stairs = N, Staircase(N, seed)
        T = self.stairs.tris
        n = T.shape[0]
        lo, hi = T.min(1), T.max(1)
        nodes = np.zeros((2 * N + 1, 8), np.uint32)

        def box(i, first, count):
            nodes[i, 0:3] = lo[first:first + count].min(0).view(np.uint32)
            nodes[i, 3:6] = hi[first:first + count].max(0).view(np.uint32)
        for k in range(N):
            box(k, 2 * k, n - 2 * k)
            nodes[k, 6], nodes[k, 7] = N + 1 + k, 0
            first, count = (2 * k, 2) if k < N - 1 else (2 * N, 1)
            box(N + 1 + k, first, count)
            nodes[N + 1 + k, 6], nodes[N + 1 + k, 7] = first, 3 | (count << 2)
        box(N, 2 * N - 2, 2)
        nodes[N, 6], nodes[N, 7] = 2 * N - 2, 3 | (2 << 2)
        self.nodes, self.order = nodes, np.arange(n, dtype=np.uint32)
        assert (np.abs(nodes[N - 1, 1:3].view(np.float32)) >= 0.6).all() and (np.abs(nodes[N - 1, 4:6].view(np.float32)) >= 0.6).all()

    def levels(self):
        return tuple(sorted({min(m, self.N) for m in LEVELS + BVH_EXTRA_LEVELS}))

    def scene(self, hprt, device=-1):
        """the device scene of the chain (hprt_scene_create takes the caller's nodes); the arrays it borrows stay on self"""
        self._P = np.ascontiguousarray(self.stairs.tris.reshape(-1, 3)); self._idx = np.arange(self._P.shape[0], dtype=np.int32)
        sh = hprt.ShapeDesc(); sh.kind = 0; sh.material = 0; sh.area_light = -1
        sh.n_tris = self._P.shape[0] // 3; sh.n_verts = self._P.shape[0]; sh.indices = self._idx.ctypes.data; sh.P = self._P.ctypes.data
        mat = hprt.MaterialDesc(); mat.type = 0; mat.Kd[:] = [.5, .5, .5]; mat.kd_texture = mat.ks_texture = mat.opacity_texture = -1
        self._shapes, self._mats = (hprt.ShapeDesc * 1)(sh), (hprt.MaterialDesc * 1)(mat)
        d = hprt.SceneDesc()
        d.nodes = self.nodes.ctypes.data; d.n_nodes = self.nodes.shape[0]; d.prim_order = self.order.ctypes.data; d.n_prims = self.order.shape[0]
        d.shapes = self._shapes; d.n_shapes = 1; d.materials = self._mats; d.n_materials = 1
        return hprt.Scene.from_desc(d, device)

    def wide(self, hprt):
        """(the four-wide records of the chain's collapse, the stack_need hprt_debug_wide_build reports)"""
        import ctypes as C
        fn = hprt.lib.hprt_debug_wide_build
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
        n_out, need = C.c_size_t(0), C.c_int(0)
        wide = np.zeros((self.nodes.shape[0], 16), np.uint32)
        assert fn(self.nodes.ctypes.data, self.nodes.shape[0], wide.ctypes.data, wide.shape[0], C.byref(n_out), C.byref(need)) == 0
        return wide[:n_out.value].copy(), need.value

    def deep_rays(self, n, seed=11):
        """(o, d, tmax, level) of the mirrored deep family.  Even i: tMax = inf (level N).  Odd i: a finite tMax that ends between the
        faces x = level - 1.6 and x = level - 0.6, for the levels of LEVELS and BVH_EXTRA_LEVELS in turn ((i % 64) // 2 % 16: each
        is the aim of 2 of every 64 consecutive rays).  Zero direction components as in the tree walks' family.  A ray that
        would pass within 1e-4 of a triangle's edge (a hundred times the float test's error at this scale) is moved in y and z until it
        does not, so that an exact point-in-triangle test and the float test of the walks cannot disagree on it."""
        N = self.N
        rng = np.random.default_rng(seed)
        i = np.arange(n)
        o = np.stack([-0.7 - rng.uniform(0, 0.2, n), rng.uniform(-0.55, 0.55, n), rng.uniform(-0.55, 0.55, n)], 1).astype(np.float32)
        end = np.stack([np.full(n, N - 0.5), rng.uniform(-0.55, 0.55, n), rng.uniform(-0.55, 0.55, n)], 1)
        scale = rng.uniform(0.5, 2.0, n)
        z = (i // 64) % 8
        aims = np.array(LEVELS + BVH_EXTRA_LEVELS)
        level = np.where(i % 2 == 0, N, np.minimum(aims[(i % 64) // 2 % len(aims)], N))
        for _ in range(64):
            d = ((end - o) * scale[:, None]).astype(np.float32)
            d[:, 1] = np.where((z == 1) | (z == 4), np.float32(0.0), np.where(z == 2, np.float32(-0.0), d[:, 1]))
            d[:, 2] = np.where((z == 3) | (z == 4), np.float32(-0.0), d[:, 2])
            near = (np.abs(self._edge_margin(o, d)) < 1e-4).any(1)
            if not near.any():
                break
            o[near, 1:] += np.float32(0.001); end[near, 1:] += 0.001
        assert not near.any() and (np.abs(o[:, 1:]) <= 0.6).all() and (np.abs(end[:, 1:]) <= 0.6).all()
        stop_x = level - 1.1
        tm = np.where(i % 2 == 0, np.inf, (stop_x - o[:, 0].astype(np.float64)) / d[:, 0].astype(np.float64)).astype(np.float32)
        return o, d, tm, level

    def _edge_margin(self, o, d):
        """[rays, triangles]: the smallest of the three edge functions of the point where the ray meets the triangle's plane
        (positive inside), in double precision"""
        T = self.stairs.tris.astype(np.float64)
        o, d = o.astype(np.float64), d.astype(np.float64)
        t = (T[None, :, 0, 0] - o[:, None, 0]) / d[:, None, 0]
        y = o[:, None, 1] + t * d[:, None, 1]; zz = o[:, None, 2] + t * d[:, None, 2]
        y0, z0 = T[None, :, 0, 1], T[None, :, 0, 2]
        w = T[None, :, 1, 1] - y0                  # the right triangle (y0, z0), (y0 + w, z0), (y0, z0 + w)
        return np.minimum(np.minimum(y - y0, zz - z0), w - (y - y0) - (zz - z0))

    def replay(self, o, d, tmax, any_hit=False):
        """BVHAccel::Intersect / IntersectP (accelerators/bvh.cpp:354-437) over the chain, statement by statement for all rays at once:
        the slab test is tests/test_wide_walk.py's; the triangle test is the exact one above (see deep_rays).  Returns (the counters
        nodes fetched, nodes entered, triangle tests, 0 summed over the rays; per ray the hit triangle or -1 — any hit: 0 / 1 —
        and the largest toVisitOffset)."""
        from test_wide_walk import slab
        nodes = self.nodes
        lo, hi = nodes[:, 0:3].view(np.float32), nodes[:, 3:6].view(np.float32)
        leaf = (nodes[:, 7] & 3) == 3
        axis, count, offset = (nodes[:, 7] & 3).astype(np.int64), (nodes[:, 7] >> 2).astype(np.int64), nodes[:, 6].astype(np.int64)
        n = tmax.shape[0]
        o = o.astype(np.float32); d = d.astype(np.float32)
        with np.errstate(all="ignore"):
            inv = (np.float32(1) / d).astype(np.float32)
        neg = inv < 0
        margin = self._edge_margin(o, d)
        tplane = ((self.stairs.tris[None, :, 0, 0].astype(np.float64) - o[:, None, 0]) / d[:, None, 0].astype(np.float64)).astype(np.float32)
        tm = tmax.astype(np.float32).copy()
        cur = np.zeros(n, np.int64); sp = np.zeros(n, np.int64); deepest = np.zeros(n, np.int64)
        stack = np.zeros((n, 64), np.int64)
        hit = np.full(n, -1, np.int64); active = np.ones(n, bool)
        fetched = entered = tests = 0
        rows = np.arange(n)
        while active.any():
            a = np.nonzero(active)[0]
            c = cur[a]
            fetched += a.shape[0]
            ok = slab(lo[c], hi[c], o[a], inv[a], neg[a], tm[a])
            entered += int(ok.sum())
            pop = ~ok
            isleaf = ok & leaf[c]
            for j in range(2):
                m = isleaf & (count[c] > j) & active[a]
                r = a[m]
                p = offset[c[m]] + j
                tests += r.shape[0]
                h = (margin[r, p] > 0) & (tplane[r, p] > 0) & (tplane[r, p] < tm[r])
                hit[r[h]] = p[h]
                if any_hit:
                    active[r[h]] = False
                else:
                    tm[r[h]] = tplane[r[h], p[h]]
            pop |= isleaf
            inner = ok & ~leaf[c]
            r = a[inner]; ci = c[inner]
            far_first = neg[r, axis[ci]]
            stack[r, sp[r]] = np.where(far_first, ci + 1, offset[ci])
            sp[r] += 1
            deepest[r] = np.maximum(deepest[r], sp[r])
            cur[r] = np.where(far_first, offset[ci], ci + 1)
            r = a[pop & active[a]]
            done = sp[r] == 0
            active[r[done]] = False
            r = r[~done]
            sp[r] -= 1
            cur[r] = stack[r, sp[r]]
        out = (hit >= 0).astype(np.uint8) if any_hit else hit
        return np.array([fetched, entered, tests, 0], np.uint64), out, deepest


def check_bvh_family(chain, n=4096):
    """The ray-family conditions for the binary chain, by the replay's largest toVisitOffset: every level is held, as the deepest
    the ray went, by at least 1/32 of the rays; every ray goes exactly as deep as aimed; some ray holds all N = 63 entries."""
    o, d, tm, level = chain.deep_rays(n)
    for any_hit in (False, True):
        _, _, deepest = chain.replay(o, d, tm, any_hit)
        if not any_hit:
            assert np.array_equal(deepest, level), int((deepest != level).sum())
        assert (deepest <= level).all()
    for m in chain.levels():
        assert (level == m).mean() >= 1 / 32, (m, (level == m).mean())
    assert level.max() == chain.N == BVH_CHAIN
    return level


def wide_depths(chain, wide, o, d, tmax):
    """per ray, the deepest stack of the four-wide walk over `wide` (the chain's collapse), replayed as tests/test_wide_walk.py
    replays it: the conservative test on the dequantised boxes, slots in the nested near / far order, every hit slot but the
    first pushed.  tMax does not shrink here: on this chain every push is made before the first leaf is reached."""
    from test_wide_walk import NONE, conservative, dequant
    qlo, qhi = dequant(wide)
    ref = wide[:, 12:16].view(np.int32)
    meta = wide[:, 3] >> 24
    out = np.zeros(tmax.shape[0], np.int64)
    for i in range(tmax.shape[0]):
        with np.errstate(all="ignore"):
            inv = (np.float32(1) / d[i]).astype(np.float32)
        neg = inv < 0
        stack, cur, deepest = [], 0, 0
        while cur is not None:
            if cur >= 0:
                ok = conservative(qlo[cur], qhi[cur], o[i], inv, neg, tmax[i]) & (ref[cur] != NONE)
                m = int(meta[cur])
                order = [0, 1, 2, 3]
                if neg[(m >> 2) & 3]: order[0], order[1] = order[1], order[0]
                if neg[(m >> 4) & 3]: order[2], order[3] = order[3], order[2]
                if neg[m & 3]: order = order[2:] + order[:2]
                hit = [s for s in order if ok[s]]
                stack += [int(ref[cur, s]) for s in reversed(hit[1:])]
                deepest = max(deepest, len(stack))
                cur = int(ref[cur, hit[0]]) if hit else (stack.pop() if stack else None)
            else:
                cur = stack.pop() if stack else None
        out[i] = deepest
    return out
