"""TAG_SHAPE_INLINE (csrc/device/dev_scene.h): BuildSceneLayout stores, in the free bits of a triangle record's tag word, what shading
reads of shapes[shape] — the SHAPE_* flags and the material index — so that k_shade requests the normals and the material as soon
as the record is there.  Checked on the host through the hprt_debug_shape_inline hook (no GPU): every triangle record either
carries exactly its shape's flags and material or has the bit clear; spheres and instances never have it; the low eight bits are
what they were before the bit existed; HPRT_INLINE_MATERIAL_MAX lowers the largest inlined material index."""
import ctypes as C
import os

import numpy as np
import pytest

from test_scene_layout import IDENT, Desc

TAG_KIND_MASK, TAG_SPHERE, TAG_INSTANCE, TAG_BOGUS, TAG_LAST, TAG_BIN_SHIFT, TAG_INST_INLINE = 3, 1, 2, 4, 8, 4, 128
TAG_SHAPE_INLINE, TAG_SHAPE_FLAGS_SHIFT, TAG_MATERIAL_SHIFT = 256, 9, 14
SHAPE_FLIP, SHAPE_HAS_N, SHAPE_HAS_UV, SHAPE_HAS_S, SHAPE_REVERSE = 1, 2, 4, 8, 16
BIN_MATTE, BIN_PLASTIC, BIN_GENERIC, BIN_SUBSTRATE = 0, 1, 2, 4

# (N, UV, S, reverse_orientation, transform_swaps_handedness) of the meshes: every SHAPE_* flag alone and together
MESH_KINDS = [(0, 0, 0, 0, 0), (1, 0, 0, 0, 0), (1, 1, 1, 0, 0), (0, 0, 0, 1, 1), (1, 0, 0, 1, 0), (0, 1, 0, 0, 1), (0, 0, 1, 0, 0), (1, 1, 1, 1, 0)]
# material types (include/hprt.h): 0 matte, 1 plastic, 3 substrate, 2 mirror -> the bins of their triangles
MATERIAL_TYPES = [0, 1, 3, 2]
MATERIAL_BINS = [BIN_MATTE, BIN_PLASTIC, BIN_SUBSTRATE, BIN_GENERIC]


class Meshes:
    """len(MESH_KINDS) x 4 quads of three triangles (the third has zero area: TAG_BOGUS), mesh k with material k % 4, and one sphere;
    one point light."""

    def __init__(self, hprt):
        self.keep = []
        n = len(MESH_KINDS) * 4
        self.shapes = (hprt.ShapeDesc * (n + 1))()
        boxes = []
        for k in range(n):
            has_n, has_uv, has_s, rev, swaps = MESH_KINDS[k // 4]
            P = np.array([[0, 0, 0], [1, 0, 0], [1, 1, .2], [0, 1, 0]], np.float32) + np.array([1.5 * k, 0, 0], np.float32)
            idx = np.array([[0, 1, 2], [0, 2, 3], [1, 1, 2]], np.int32)
            N = np.tile(np.array([[0, 0, 1]], np.float32), (4, 1)); UV = P[:, :2].copy(); S = np.tile(np.array([[1, 0, 0]], np.float32), (4, 1))
            self.keep += [P, idx, N, UV, S]
            sh = self.shapes[k]
            sh.kind = 0; sh.material = k % 4; sh.area_light = -1; sh.reverse_orientation = rev; sh.transform_swaps_handedness = swaps
            sh.n_tris = 3; sh.n_verts = 4; sh.indices = idx.ctypes.data; sh.P = P.ctypes.data
            sh.N = N.ctypes.data if has_n else None; sh.UV = UV.ctypes.data if has_uv else None; sh.S = S.ctypes.data if has_s else None
            boxes += [(P[t].min(axis=0), P[t].max(axis=0)) for t in idx]
        sph = self.shapes[n]
        sph.kind = 1; sph.material = 2; sph.area_light = -1
        sph.object_to_world[:] = IDENT; sph.world_to_object[:] = IDENT
        sph.radius, sph.z_min, sph.z_max, sph.theta_min, sph.theta_max, sph.phi_max = 1, -1, 1, 0, np.pi, 2 * np.pi
        boxes.append((np.array([-1, -1, -1], np.float32), np.array([1, 1, 1], np.float32)))
        self.mats = (hprt.MaterialDesc * 4)()
        for m, t in enumerate(MATERIAL_TYPES):
            self.mats[m].type = t; self.mats[m].Kd[:] = [.5, .5, .5]; self.mats[m].Ks[:] = [.2, .2, .2]; self.mats[m].roughness = .1
            self.mats[m].kd_texture = self.mats[m].ks_texture = self.mats[m].opacity_texture = -1
        self.lights = (hprt.LightDesc * 1)()
        l = self.lights[0]
        l.type = 0; l.I[:] = [1, 1, 1]; l.shape = -1; l.texture = -1; l.pos[:] = [0, 0, 2]; l.light_to_world[:] = IDENT; l.world_to_light[:] = IDENT
        self.nodes, self.order = Desc._bvh(hprt, boxes)
        d = hprt.SceneDesc()
        d.nodes = self.nodes.ctypes.data; d.n_nodes = self.nodes.shape[0]
        d.prim_order = self.order.ctypes.data; d.n_prims = self.order.shape[0]
        d.shapes = self.shapes; d.n_shapes = n + 1
        d.materials = self.mats; d.n_materials = 4
        d.lights = self.lights; d.n_lights = 1
        self.d = d
        # creation order: (shape, triangle or -1 for the sphere)
        self.prims = [(k, t) for k in range(n) for t in range(3)] + [(n, -1)]


def layout(hprt, d):
    fn = hprt.lib.hprt_debug_shape_inline
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    n_prims, n_shapes = C.c_size_t(), C.c_size_t()
    assert fn(C.byref(d), None, None, 0, C.byref(n_prims), None, None, 0, C.byref(n_shapes)) == 0, hprt.lib.hprt_last_error().decode()
    tags, shape = np.zeros(n_prims.value, np.uint32), np.zeros(n_prims.value, np.uint32)
    flags, material = np.zeros(n_shapes.value, np.uint32), np.zeros(n_shapes.value, np.int32)
    assert fn(C.byref(d), tags.ctypes.data, shape.ctypes.data, tags.size, C.byref(n_prims), flags.ctypes.data, material.ctypes.data, flags.size,
              C.byref(n_shapes)) == 0
    return tags, shape, flags, material


def last_of_leaf(nodes, n_prims):
    """per ordered primitive of one aggregate: is it the last of its leaf (TAG_LAST)"""
    last = np.zeros(n_prims, bool)
    for nd in nodes:
        if (nd[7] & 3) == 3:
            last[int(nd[6]) + (int(nd[7]) >> 2) - 1] = True
    return last


def check_records(tags, shape, flags, material, is_triangle, inline_max=(1 << 18) - 1):
    for i in range(tags.size):
        tag = int(tags[i])
        if not is_triangle[i]:
            assert (tag >> 8) == 0, (i, hex(tag))      # spheres and instances: nothing above bit 7
            continue
        s = int(shape[i])
        if int(material[s]) <= inline_max:
            assert tag & TAG_SHAPE_INLINE, (i, hex(tag))
            assert (tag >> TAG_SHAPE_FLAGS_SHIFT) & 31 == int(flags[s]) & 31, (i, hex(tag), int(flags[s]))
            assert tag >> TAG_MATERIAL_SHIFT == int(material[s]), (i, hex(tag), int(material[s]))
        else:
            assert (tag >> 8) == 0, (i, hex(tag))      # the bit is clear and nothing else changes


def test_every_triangle_record_carries_its_shape(hprt):
    s = Meshes(hprt)
    tags, shape, flags, material = layout(hprt, s.d)
    assert tags.size == len(s.prims)
    # the shapes' flags, as BuildSceneLayout derives them from the description
    for k, (has_n, has_uv, has_s, rev, swaps) in enumerate(MESH_KINDS):
        want = (SHAPE_FLIP if rev ^ swaps else 0) | (SHAPE_HAS_N if has_n else 0) | (SHAPE_HAS_UV if has_uv else 0) | (SHAPE_HAS_S if has_s else 0) | (SHAPE_REVERSE if rev else 0)
        assert [int(f) for f in flags[4 * k:4 * k + 4]] == [want] * 4
    assert len(set(int(f) for f in flags[:-1])) == len(MESH_KINDS) and max(int(f) for f in flags) < 32
    ordered = [s.prims[int(o)] for o in s.order]
    is_triangle = np.array([t >= 0 for _, t in ordered])
    check_records(tags, shape, flags, material, is_triangle)
    assert (tags[is_triangle] & TAG_SHAPE_INLINE).all()
    # bits 0-7: kind, bogus, last of its leaf, bin — what they were before the tag carried anything else
    last = last_of_leaf(s.nodes, tags.size)
    for i, (k, t) in enumerate(ordered):
        if t < 0:
            want = TAG_SPHERE | (BIN_GENERIC << TAG_BIN_SHIFT)
        else:
            assert int(shape[i]) == k
            want = (TAG_BOGUS if t == 2 else 0) | (MATERIAL_BINS[k % 4] << TAG_BIN_SHIFT)
        want |= TAG_LAST if last[i] else 0
        assert int(tags[i]) & 0xff == want, (i, k, t, hex(int(tags[i])), hex(want))


def test_spheres_and_instances_never_carry_it(hprt):
    s = Desc(hprt, instanced=True)      # top level: the two-triangle mesh and one instance of an object holding the unit sphere
    tags, shape, flags, material = layout(hprt, s.d)
    kinds = [int(t) & TAG_KIND_MASK for t in tags]
    assert sorted(kinds) == [0, 0, TAG_SPHERE, TAG_INSTANCE]
    check_records(tags, shape, flags, material, np.array([k == 0 for k in kinds]))
    for t, k in zip(tags, kinds):
        assert bool(int(t) & TAG_SHAPE_INLINE) == (k == 0)
        if k == TAG_INSTANCE:
            assert int(t) & 0xff == TAG_INSTANCE | TAG_INST_INLINE | TAG_LAST      # (an identity instance: affine, its matrix inline; a leaf of its own)


def test_material_index_past_the_inline_maximum_keeps_the_lookup(hprt):
    s = Meshes(hprt)
    full = layout(hprt, s.d)
    os.environ["HPRT_INLINE_MATERIAL_MAX"] = "1"
    try:
        tags, shape, flags, material = layout(hprt, s.d)
    finally:
        del os.environ["HPRT_INLINE_MATERIAL_MAX"]
    assert np.array_equal(flags, full[2]) and np.array_equal(material, full[3]) and np.array_equal(shape, full[1])
    assert np.array_equal(tags & 0xff, full[0] & 0xff)
    is_triangle = (tags & TAG_KIND_MASK) == 0
    check_records(tags, shape, flags, material, is_triangle, inline_max=1)
    mat_of = material[shape[is_triangle]]
    inlined = (tags[is_triangle] & TAG_SHAPE_INLINE) != 0
    assert np.array_equal(inlined, mat_of <= 1) and inlined.any() and (~inlined).any()
    assert set(int(m) for m in mat_of) == {0, 1, 2, 3}


def test_the_override_can_only_lower_the_maximum(hprt):
    s = Meshes(hprt)
    full = layout(hprt, s.d)
    os.environ["HPRT_INLINE_MATERIAL_MAX"] = str(1 << 30)
    try:
        tags = layout(hprt, s.d)[0]
    finally:
        del os.environ["HPRT_INLINE_MATERIAL_MAX"]
    assert np.array_equal(tags, full[0])
