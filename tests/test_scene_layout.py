"""BuildSceneLayout (csrc/scene_layout.cpp): every check hprt_scene_create makes of an HprtSceneDesc, one case per error, each on
a small valid description with a single defect.  The checks run before a device is chosen, so these cases hold with or without
a GPU.  Also CheckBvhNodes behind the hprt_debug_wide_build hook.

Not reached here: the two limits that need gigabytes of input (more than 89,478,485 primitives or 67,108,863 interior nodes
over all aggregates; infinite-light tables of more than 2^31 floats)."""
import ctypes as C

import numpy as np
import pytest

IDENT = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]


class ObjectDesc(C.Structure):
    _fields_ = [("first_shape", C.c_uint32), ("n_shapes", C.c_uint32), ("nodes", C.c_void_p), ("n_nodes", C.c_uint32),
                ("prim_order", C.c_void_p), ("n_prims", C.c_uint32)]


class InstanceDesc(C.Structure):
    _fields_ = [("object", C.c_int32), ("instance_to_world", C.c_float * 16), ("world_to_instance", C.c_float * 16)]


class TopItem(C.Structure):
    _fields_ = [("kind", C.c_int32), ("index", C.c_uint32)]


class Desc:
    """A valid description: shape 0 a two-triangle mesh, shape 1 a unit sphere, one matte material, three point lights, two 1x1
    textures.  instanced: the sphere is object 0's, instanced once; top: explicit top-level items (kind, index)."""

    def __init__(self, hprt, instanced=False, top=None):
        self.P = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], np.float32)
        self.idx = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
        mesh = hprt.ShapeDesc(); mesh.kind = 0; mesh.material = 0; mesh.area_light = -1
        mesh.n_tris = 2; mesh.n_verts = 4; mesh.indices = self.idx.ctypes.data; mesh.P = self.P.ctypes.data
        sph = hprt.ShapeDesc(); sph.kind = 1; sph.material = 0; sph.area_light = -1
        sph.object_to_world[:] = IDENT; sph.world_to_object[:] = IDENT
        sph.radius, sph.z_min, sph.z_max, sph.theta_min, sph.theta_max, sph.phi_max = 1, -1, 1, 0, np.pi, 2 * np.pi
        self.shapes = (hprt.ShapeDesc * 2)(mesh, sph)
        mat = hprt.MaterialDesc(); mat.type = 0; mat.Kd[:] = [.5, .5, .5]; mat.kd_texture = mat.ks_texture = mat.opacity_texture = -1
        self.mats = (hprt.MaterialDesc * 1)(mat)
        self.lights = (hprt.LightDesc * 3)()
        for l in self.lights:
            l.type = 0; l.I[:] = [1, 1, 1]; l.shape = -1; l.texture = -1; l.pos[:] = [0, 0, 2]
            l.light_to_world[:] = IDENT; l.world_to_light[:] = IDENT
        self.texel = np.array([.5, .6, .9], np.float32); self.lut = np.zeros(128, np.float32); self.lut2 = np.ones(128, np.float32)
        self.levels = (hprt.TextureLevel * 2)()
        self.texs = (hprt.TextureDesc * 2)()
        for k in range(2):
            self.levels[k].w = self.levels[k].h = 1; self.levels[k].rgb = self.texel.ctypes.data
            t = self.texs[k]; t.levels = C.pointer(self.levels[k]); t.n_levels = 1; t.max_anisotropy = 8; t.su = t.sv = 1
            t.weight_lut = self.lut.ctypes.data
        sphere_box = (np.array([-1, -1, -1], np.float32), np.array([1, 1, 1], np.float32))
        boxes = {0: [(self.P[t].min(axis=0), self.P[t].max(axis=0)) for t in self.idx], 1: [sphere_box]}
        d = hprt.SceneDesc()
        if instanced:
            self.onodes, self.oorder = self._bvh(hprt, [sphere_box])
            self.objects = (ObjectDesc * 2)()
            self.objects[0] = ObjectDesc(1, 1, self.onodes.ctypes.data, self.onodes.shape[0], self.oorder.ctypes.data, self.oorder.shape[0])
            self.instances = (InstanceDesc * 1)()
            self.instances[0].object = 0; self.instances[0].instance_to_world[:] = IDENT; self.instances[0].world_to_instance[:] = IDENT
            top = [(0, 0), (1, 0)]
            d.objects = C.cast(self.objects, C.c_void_p); d.n_objects = 1
            d.instances = C.cast(self.instances, C.c_void_p); d.n_instances = 1
        if top is not None:
            self.top = (TopItem * len(top))(*[TopItem(k, i) for k, i in top])
            d.top = C.cast(self.top, C.c_void_p); d.n_top = len(top)
            prim_boxes = [b for k, i in top for b in (boxes[i] if k == 0 else [sphere_box])]
        else:
            prim_boxes = boxes[0] + boxes[1]
        self.nodes, self.order = self._bvh(hprt, prim_boxes)
        d.nodes = self.nodes.ctypes.data; d.n_nodes = self.nodes.shape[0]
        d.prim_order = self.order.ctypes.data; d.n_prims = self.order.shape[0]
        d.shapes = self.shapes; d.n_shapes = 2
        d.materials = self.mats; d.n_materials = 1
        d.lights = self.lights; d.n_lights = 3
        d.textures = C.cast(self.texs, C.c_void_p); d.n_textures = 2
        self.d = d

    @staticmethod
    def _bvh(hprt, boxes):
        nodes, order = hprt.Bvh.from_bounds(np.array([b[0] for b in boxes], np.float32), np.array([b[1] for b in boxes], np.float32)).arrays()
        return nodes, order

    def node(self, leaf):
        """index of the first leaf (or interior node) of the top-level tree"""
        return int(np.nonzero(((self.nodes[:, 7] & 3) == 3) == leaf)[0][0])


def create(hprt, s):
    h = C.c_void_p()
    rc = hprt.lib.hprt_scene_create(C.byref(s.d), -1, C.byref(h))
    if rc == 0:
        hprt.lib.hprt_scene_destroy(h)
    return rc, hprt.lib.hprt_last_error().decode()


def _set(obj, **kw):
    for k, v in kw.items():
        setattr(obj, k, v)


def _emissive_mesh(s, first=0):
    s.shapes[0].area_light = first
    for l in (first, first + 1):
        _set(s.lights[l], type=2, shape=0)


def _deep_tree(s):
    """a chain of 65 interior nodes over the mesh, now of 65 triangles, and the sphere: depth 66, deeper than the 64-entry stack"""
    s.idx = np.tile(np.array([[0, 1, 2]], np.int32), (65, 1))
    _set(s.shapes[0], n_tris=65, indices=s.idx.ctypes.data)
    s.nodes = np.zeros((131, 8), np.uint32)
    s.nodes[:, 0:3] = np.array([-1, -1, -1], np.float32).view(np.uint32); s.nodes[:, 3:6] = np.array([1, 1, 1], np.float32).view(np.uint32)
    s.nodes[:, 7] = 3 | (1 << 2)                        # leaves of one primitive ...
    s.nodes[:65, 7] = 1 << 2                            # ... but for the chain: node i's first child is i + 1, its second the leaf 66 + i
    s.nodes[:65, 6] = 66 + np.arange(65)
    s.nodes[65:, 6] = np.arange(66)
    s.order = np.arange(66, dtype=np.uint32)
    _set(s.d, nodes=s.nodes.ctypes.data, n_nodes=131, prim_order=s.order.ctypes.data, n_prims=66)


# (name, description variant, defect, code, message fragment): one per error of BuildSceneLayout
CASES = [
    # arrays
    ("null_shapes", {}, lambda s: _set(s.d, shapes=None), "E_INVALID", "null array with non-zero count"),
    ("null_textures", {}, lambda s: _set(s.d, textures=None), "E_INVALID", "null texture array"),
    ("null_objects", {"instanced": True}, lambda s: _set(s.d, objects=None), "E_INVALID", "null instancing array"),
    # shapes
    ("shape_material", {}, lambda s: _set(s.shapes[0], material=1), "E_INVALID", "shape material index out of range"),
    ("shape_area_light", {}, lambda s: _set(s.shapes[1], area_light=3), "E_INVALID", "shape area light index out of range"),
    ("mesh_without_P", {}, lambda s: _set(s.shapes[0], P=None), "E_INVALID", "mesh without indices or positions"),
    ("mesh_vertex_index", {}, lambda s: s.idx.__setitem__((1, 2), 4), "E_INVALID", "mesh vertex index out of range"),
    ("emissive_mesh_lights_past_table", {}, lambda s: _set(s.shapes[0], area_light=2), "E_INVALID", "exceed the light table"),
    ("emissive_mesh_not_its_lights", {}, lambda s: _set(s.shapes[0], area_light=0), "E_INVALID", "must be the diffuse area light of its triangle"),
    ("shape_kind", {}, lambda s: _set(s.shapes[1], kind=2), "E_INVALID", "unknown shape kind"),
    ("vertices_past_2_32", {}, lambda s: (_set(s.shapes[0], n_verts=0xffffffff), _set(s.shapes[1], kind=0, n_tris=0, n_verts=1)),
     "E_UNSUPPORTED", "more than 2^32 vertices"),
    # aggregates
    ("object_shape_range", {"instanced": True}, lambda s: _set(s.objects[0], n_shapes=2), "E_INVALID", "object shape range out of bounds"),
    ("object_without_nodes", {"instanced": True}, lambda s: _set(s.objects[0], nodes=None), "E_INVALID", "object without its aggregate arrays"),
    ("shape_in_two_objects", {"instanced": True}, lambda s: (s.objects.__setitem__(1, s.objects[0]), _set(s.d, n_objects=2)),
     "E_INVALID", "a shape belongs to two objects"),
    ("area_light_in_object", {"instanced": True}, lambda s: _set(s.shapes[1], area_light=0), "E_UNSUPPORTED", "not supported with object instancing"),
    ("instance_object", {"instanced": True}, lambda s: _set(s.instances[0], object=1), "E_INVALID", "instance object index out of range"),
    ("instance_of_empty_object", {"instanced": True}, lambda s: _set(s.objects[0], n_shapes=0), "E_INVALID", "instance of an empty object"),
    ("top_item_object_shape", {"instanced": True}, lambda s: _set(s.top[0], index=1), "E_INVALID", "missing or object-owned shape"),
    ("top_item_instance", {"instanced": True}, lambda s: _set(s.top[1], index=1), "E_INVALID", "top-level item references a missing instance"),
    ("top_item_kind", {"instanced": True}, lambda s: _set(s.top[0], kind=2), "E_INVALID", "unknown top-level item kind"),
    ("instances_without_top", {"instanced": True}, lambda s: _set(s.d, top=None, n_top=0), "E_INVALID", "instances need the top-level item list"),
    ("prim_order_length", {}, lambda s: _set(s.d, n_prims=2), "E_INVALID", "prim_order length"),
    ("bvh_leaf_empty", {}, lambda s: s.nodes.__setitem__((s.node(True), 7), 3), "E_INVALID", "a BVH leaf is empty"),
    ("bvh_leaf_range", {}, lambda s: s.nodes.__setitem__((s.node(True), 6), 3), "E_INVALID", "a BVH leaf references primitives out of range"),
    ("bvh_second_child_past_end", {}, lambda s: s.nodes.__setitem__((s.node(False), 6), s.nodes.shape[0]), "E_INVALID", "second child is out of range"),
    ("bvh_second_child_not_after", {}, lambda s: s.nodes.__setitem__((s.node(False), 6), s.node(False)), "E_INVALID", "second child is out of range"),
    ("bvh_interior_last", {}, lambda s: s.nodes.__setitem__((-1, 7), 1 << 2), "E_INVALID", "the last BVH node is an interior node"),
    ("nodes_without_prims", {}, lambda s: _set(s.d, n_nodes=0), "E_INVALID", "aggregate with primitives but no nodes"),
    ("prim_order_entry", {}, lambda s: s.order.__setitem__(0, 3), "E_INVALID", "prim_order entry out of range"),
    ("bvh_too_deep", {}, _deep_tree, "E_UNSUPPORTED", "BVH deeper than the 64-entry traversal stack"),
    # lights
    ("light_type", {}, lambda s: _set(s.lights[0], type=4), "E_INVALID", "unknown light type"),
    ("infinite_map_index", {}, lambda s: _set(s.lights[0], type=3, texture=2), "E_INVALID", "infinite light: map index out of range"),
    ("infinite_map_wrap", {}, lambda s: (_set(s.lights[0], type=3, texture=0), _set(s.texs[0], wrap=1)), "E_INVALID", "repeat-wrapped pyramid"),
    ("infinite_map_size", {}, lambda s: (_set(s.lights[0], type=3, texture=0), _set(s.levels[0], w=1 << 14, h=1 << 13)),
     "E_UNSUPPORTED", "infinite light: map larger than 2^26 texels"),
    ("area_light_shape", {}, lambda s: _set(s.lights[0], type=2, shape=2), "E_INVALID", "area light shape out of range"),
    ("area_light_not_its_shape", {}, lambda s: _set(s.lights[0], type=2, shape=1), "E_INVALID", "do not reference each other"),
    ("light_strategy", {}, lambda s: _set(s.d, light_strategy=3), "E_INVALID", "light_strategy must be"),
    # materials, textures
    ("material_type", {}, lambda s: _set(s.mats[0], type=7), "E_UNSUPPORTED", "material type outside the hot-path scope"),
    ("material_texture", {}, lambda s: _set(s.mats[0], kd_texture=2), "E_INVALID", "material texture index out of range"),
    ("texture_without_lut", {}, lambda s: _set(s.texs[1], weight_lut=None), "E_INVALID", "texture without levels or weight table"),
    ("texture_wrap", {}, lambda s: _set(s.texs[0], wrap=3), "E_INVALID", "texture wrap mode out of range"),
    ("texture_level_empty", {}, lambda s: _set(s.levels[1], w=0), "E_INVALID", "empty texture level"),
    ("texture_floats_past_2_32", {}, lambda s: _set(s.levels[0], w=40000, h=40000), "E_UNSUPPORTED", "more than 2^32 texture floats"),
    ("texture_luts_differ", {}, lambda s: _set(s.texs[1], weight_lut=s.lut2.ctypes.data), "E_INVALID", "disagree on the EWA weight table"),
    # an emissive mesh the top-level item list leaves out
    ("emissive_triangle_outside_top", {"top": [(0, 1)]}, _emissive_mesh, "E_UNSUPPORTED", "emissive triangle outside the top-level aggregate"),
]


VALID = [("plain", {}, lambda s: None), ("instanced", {"instanced": True}, lambda s: None), ("top_list", {"top": [(0, 1)]}, lambda s: None),
         ("emissive_mesh", {}, _emissive_mesh), ("infinite_light", {}, lambda s: _set(s.lights[0], type=3, texture=0)),
         ("spatial", {}, lambda s: _set(s.d, light_strategy=2))]


@pytest.mark.parametrize("name,variant,change", VALID, ids=[v[0] for v in VALID])
def test_the_descriptions_the_cases_start_from_are_valid(hprt, name, variant, change):
    s = Desc(hprt, **variant)
    change(s)
    rc, msg = create(hprt, s)
    assert rc in (0, hprt.E_NO_DEVICE), msg      # (no device: the layout was built, the upload refused)


@pytest.mark.parametrize("name,variant,defect,code,fragment", CASES, ids=[c[0] for c in CASES])
def test_a_single_defect_is_reported_before_the_device_is_chosen(hprt, name, variant, defect, code, fragment):
    s = Desc(hprt, **variant)
    defect(s)
    rc, msg = create(hprt, s)
    assert rc == getattr(hprt, code) and fragment in msg, (rc, msg)


def test_a_null_description_is_refused(hprt):
    h = C.c_void_p()
    assert hprt.lib.hprt_scene_create(None, -1, C.byref(h)) == hprt.E_INVALID
    assert "null argument" in hprt.lib.hprt_last_error().decode()


# ---- hprt_debug_wide_build: CheckBvhNodes before BuildWide ----
@pytest.fixture(scope="module")
def wide_build(hprt):
    fn = hprt.lib.hprt_debug_wide_build
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
    rng = np.random.default_rng(7)
    lo = rng.uniform(-1, 1, (40, 3)).astype(np.float32)
    nodes, _ = hprt.Bvh.from_bounds(lo, lo + np.float32(.1)).arrays()
    n_out, need = C.c_size_t(0), C.c_int(0)
    return lambda a: fn(a.ctypes.data, a.shape[0], None, 0, C.byref(n_out), C.byref(need)), nodes


def test_the_wide_build_hook_rejects_malformed_node_arrays(hprt, wide_build):
    build, nodes = wide_build
    assert build(nodes) == 0
    interior = int(np.nonzero((nodes[:, 7] & 3) != 3)[0][1]); leaf = int(np.nonzero((nodes[:, 7] & 3) == 3)[0][0])
    for i, word, value, fragment in [(interior, 6, nodes.shape[0], "second child"),       # past the end
                                     (interior, 6, interior, "second child"),             # not after the node
                                     (nodes.shape[0] - 1, 7, 1 << 2, "last BVH node"),    # an interior last node
                                     (leaf, 7, 3, "leaf is empty")]:
        bad = nodes.copy()
        bad[i, word] = value
        assert build(bad) == hprt.E_INVALID, (i, word, value)
        assert fragment in hprt.lib.hprt_last_error().decode()
