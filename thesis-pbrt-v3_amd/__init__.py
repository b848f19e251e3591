"""hprt — Python (ctypes) binding of the C ABI in include/hprt.h.

Host-side mirror of the pbrt plugin surface for the one hot path this package
accelerates:

    Model   <- pbrtParseFile / api.cpp state          (core/parser.cpp, core/api.cpp)
    Bvh     <- CreateBVHAccelerator / BVHAccel ctor   (accelerators/bvh.cpp:155-185,529-535)
    KdTree  <- CreateKdTreeAccelerator / buildTree    (accelerators/kdtreeaccel.cpp:212-380,523-545)
    Rbsp    <- CreateRBSPTreeAccelerator / buildTree  (accelerators/rbsp.cpp:181-403,549-571)
    RbspKd  <- CreateRBSPKdTreeAccelerator / buildTree (accelerators/rbspKd.cpp:194-488,640-665)
    BspPaper <- CreateBSPPaperTreeAccelerator / buildTree (accelerators/bspPaper.cpp:34-319)
    BspPaperKd <- CreateBSPPaperKdTreeAccelerator / buildTree (accelerators/bspPaperKd.cpp:34-353)
    BspNode, BspNodeKd <- Create{BSPArbitrary,BSPCluster,BSPRandom}{,WithKd,FastKd}TreeAccelerator / buildTree
               (accelerators/bspNodeBased.cpp:27-223, bspNodeBasedWithKd.cpp, bspNodeBasedFastKd.cpp:28-330)
    Scene   <- Scene + BVHAccel::Intersect/IntersectP (accelerators/bvh.cpp:354-437)
               and SamplerIntegrator::Render with PathIntegrator::Li
               (core/integrator.cpp:230-360, integrators/path.cpp:64-204)

The shared library is built in-tree by build.py (hipcc, gfx950).  There is no CPU
fallback: device calls raise HprtError when no GPU is present, and importing this
package raises if the library is missing.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HPRT_LIB") or os.path.join(_HERE, "lib", "libhprt.so")      # HPRT_LIB: another build of the same library (tools/build_variant.sh, A/B measurements)


class HprtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("hprt error %d: %s" % (code, msg))
        self.code = code


E_INVALID, E_IO, E_PARSE, E_NO_DEVICE, E_DEVICE, E_UNSUPPORTED = -1, -2, -3, -4, -5, -6
RENDER_COUNT_WORK = 1
RENDER_PIXEL_STATS = 2
RENDER_COUNT_TRACED = 4
RENDER_TRACE_ALL = 8
RENDER_EXPORT_FOREIGN = 16
ACCEL_BVH, ACCEL_KDTREE, ACCEL_RBSP = 0, 1, 2
ACCEL_BSP = ACCEL_RBSP      # the general BSP tree (bsppaper): its interior nodes are bspTreeNodeTraversals too
KD_MAX_DEPTH = 64        # HPRT_KD_MAX_DEPTH: the kd walk's todo capacity
RBSP_MAX_DEPTH = 64      # HPRT_RBSP_MAX_DEPTH: the RBSP walk's todo capacity
COMM_ID_BYTES = 128
# HprtFilmRecord: one cross-tile film contribution (include/hprt.h)
FILM_RECORD = np.dtype([("dest_pixel", np.uint32), ("src_tile", np.uint32), ("xyz", np.float32, 3), ("weight", np.float32)])
assert FILM_RECORD.itemsize == 24


class RenderOptions(C.Structure):
    _fields_ = [
        ("xres", C.c_int32), ("yres", C.c_int32), ("crop", C.c_float * 4), ("filter_radius", C.c_float * 2),
        ("film_scale", C.c_float), ("max_sample_luminance", C.c_float),
        ("fov", C.c_float), ("lens_radius", C.c_float), ("focal_distance", C.c_float),
        ("screen_window", C.c_float * 4), ("camera_to_world", C.c_float * 16), ("world_to_camera", C.c_float * 16),
        ("spp", C.c_int32), ("sample_pixel_center", C.c_int32), ("max_depth", C.c_int32), ("rr_threshold", C.c_float),
        ("light_strategy", C.c_int32), ("max_node_prims", C.c_int32), ("isect_cost", C.c_int32), ("trav_cost", C.c_int32),
    ]

    def copy(self):
        o = RenderOptions()
        C.memmove(C.byref(o), C.byref(self), C.sizeof(RenderOptions))
        return o

    def film_bounds(self):
        """croppedPixelBounds (core/film.cpp:56-60) as (x0, y0, x1, y1)."""
        f32 = np.float32
        x0 = int(np.ceil(f32(self.xres) * f32(self.crop[0])))
        x1 = int(np.ceil(f32(self.xres) * f32(self.crop[1])))
        y0 = int(np.ceil(f32(self.yres) * f32(self.crop[2])))
        y1 = int(np.ceil(f32(self.yres) * f32(self.crop[3])))
        return x0, y0, x1, y1


class RenderDesc(C.Structure):
    _fields_ = [("opt", RenderOptions), ("tile_begin", C.c_int32), ("tile_end", C.c_int32), ("tile_stride", C.c_int32),
                ("spp_chunk", C.c_int32), ("flags", C.c_int32)]


class AoParams(C.Structure):
    """HprtAoParams: CreateAOIntegrator's "nsamples" and "cossample" (integrators/ao.cpp:105-126)."""
    _fields_ = [("n_samples", C.c_int32), ("cos_sample", C.c_int32)]


class DirectParams(C.Structure):
    """HprtDirectParams: CreateDirectLightingIntegrator's "strategy" (0 all, 1 one) and "maxdepth" (integrators/directlighting.cpp:102-135)."""
    _fields_ = [("strategy", C.c_int32), ("max_depth", C.c_int32)]


DIRECT_MAX_DEPTH = 8      # HPRT_DIRECT_MAX_DEPTH


class RenderStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "camera_rays", "rays", "shadow_rays", "nodes_fetched", "nodes_fetched_p", "nodes_entered", "nodes_entered_p",
        "tri_tests", "tri_tests_p", "sphere_tests", "sphere_tests_p")] + [
        ("render_seconds", C.c_double), ("extend_seconds", C.c_double), ("occluded_seconds", C.c_double),
        ("extend_launches", C.c_uint64), ("occluded_launches", C.c_uint64), ("extend_rays", C.c_uint64), ("occluded_rays", C.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# ---- HprtSceneDesc and its parts (include/hprt.h): what a pbrt-side adapter fills from the primitives it was given ----
class ShapeDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("material", C.c_int32), ("area_light", C.c_int32),
                ("reverse_orientation", C.c_int32), ("transform_swaps_handedness", C.c_int32),
                ("n_tris", C.c_uint32), ("n_verts", C.c_uint32),
                ("indices", C.c_void_p), ("P", C.c_void_p), ("N", C.c_void_p), ("UV", C.c_void_p), ("S", C.c_void_p),
                ("object_to_world", C.c_float * 16), ("world_to_object", C.c_float * 16),
                ("radius", C.c_float), ("z_min", C.c_float), ("z_max", C.c_float), ("theta_min", C.c_float), ("theta_max", C.c_float),
                ("phi_max", C.c_float)]


class MaterialDesc(C.Structure):
    _fields_ = [("type", C.c_int32), ("Kd", C.c_float * 3), ("sigma", C.c_float), ("Ks", C.c_float * 3), ("roughness", C.c_float),
                ("remap_roughness", C.c_int32), ("kd_texture", C.c_int32), ("ks_texture", C.c_int32),
                ("Kr", C.c_float * 3), ("Kt", C.c_float * 3), ("opacity", C.c_float * 3), ("eta", C.c_float), ("opacity_texture", C.c_int32)]


class TextureLevel(C.Structure):
    _fields_ = [("w", C.c_int32), ("h", C.c_int32), ("rgb", C.c_void_p)]


class TextureDesc(C.Structure):
    _fields_ = [("levels", C.POINTER(TextureLevel)), ("n_levels", C.c_uint32), ("trilinear", C.c_int32), ("max_anisotropy", C.c_float),
                ("wrap", C.c_int32), ("su", C.c_float), ("sv", C.c_float), ("du", C.c_float), ("dv", C.c_float), ("weight_lut", C.c_void_p)]


class LightDesc(C.Structure):
    _fields_ = [("type", C.c_int32), ("pos", C.c_float * 3), ("I", C.c_float * 3), ("shape", C.c_int32), ("two_sided", C.c_int32),
                ("texture", C.c_int32), ("light_to_world", C.c_float * 16), ("world_to_light", C.c_float * 16)]


class RbspKdParams(C.Structure):
    """HprtRbspKdParams: CreateRBSPKdTreeAccelerator's parameters plus the builder's thread count."""
    _fields_ = [("isect_cost", C.c_int), ("trav_cost", C.c_int), ("kd_trav_cost", C.c_int), ("empty_bonus", C.c_float), ("max_prims", C.c_int),
                ("max_depth", C.c_int), ("n_directions", C.c_int), ("threads", C.c_int)]


class BuildDeviceOpts(C.Structure):
    """HprtBuildDeviceOpts: the device-assisted RBSP / RBSPKd build (0 = default)."""
    _fields_ = [("device", C.c_int), ("min_candidates", C.c_uint32), ("max_edges", C.c_uint32)]


class BuildDeviceStats(C.Structure):
    """HprtBuildDeviceStats"""
    _fields_ = [("nodes_device", C.c_uint64), ("candidates_device", C.c_uint64), ("candidates_recosted_on_host", C.c_uint64),
                ("nodes_host", C.c_uint64), ("seconds_device", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class BspBuildDeviceOpts(C.Structure):
    """HprtBspBuildDeviceOpts: the device-assisted BspPaper / BspPaperKd build (0 = default)."""
    _fields_ = [("device", C.c_int), ("min_candidates", C.c_uint32), ("max_edges", C.c_uint32), ("max_faces", C.c_uint32),
                ("max_face_edges", C.c_uint32), ("max_stack", C.c_uint32)]


def _device_opts(Opts, device, *fields):
    """The options of a device-assisted build (BuildDeviceOpts or BspBuildDeviceOpts), or None for a host build (device None)"""
    return None if device is None else Opts(int(device), *fields)


def _build_tree(prefix, how, head, prm, opts):
    """hprt_<prefix>_<how> or, with opts (_device_opts) not None, hprt_<prefix>_<how>_device: (handle, build stats dict or None)"""
    h = C.c_void_p()
    if opts is None:
        _check(getattr(lib, "hprt_%s_%s" % (prefix, how))(*head, prm, C.byref(h)))
        return h, None
    st = BuildDeviceStats()
    _check(getattr(lib, "hprt_%s_%s_device" % (prefix, how))(*head, prm, C.byref(opts), C.byref(st), C.byref(h)))
    return h, st.as_dict()


class _Tree:
    """A host tree handle (KdTree, Rbsp, RbspKd, BspPaper, BspPaperKd) over the C calls hprt_<_prefix>_info / _copy / _destroy: info() names the info
    words `_info_keys`; the copy of the RBSP trees takes a direction table as well (M in info)."""
    _prefix = None
    _info_keys = ()

    def _call(self, name, *args):
        _check(getattr(lib, "hprt_%s_%s" % (self._prefix, name))(self._h, *args))

    def info(self):
        i = (C.c_uint32 * len(self._info_keys))()
        self._call("info", i)
        return dict(zip(self._info_keys, i))

    def arrays(self):
        """(nodes [n, 2] uint32: word 0 split / onePrimitive / primitiveIndicesOffset, word 1 flags; prim_indices uint32)"""
        inf = self.info()
        nodes = np.zeros((inf["nodes"], 2), np.uint32)
        idx = np.zeros(inf["prim_refs"], np.uint32)
        self._call("copy", _ptr(nodes), _ptr(idx), *([None] if "M" in inf else []))
        return nodes, idx

    @classmethod
    def _from_arrays(cls, nodes, prim_indices, n_prims, bounds, *head):
        """The handle of a tree made by hand (diagnostics hook hprt_debug_<_prefix>_from_arrays, not part of include/hprt.h): nodes
        and prim_indices as arrays() gives them, n_prims the primitives the tree is over, bounds its six floats pMin, pMax; head:
        the arguments in front (M).  The tree passes the checks a built tree passes (HprtError E_INVALID / E_UNSUPPORTED)."""
        nodes = np.ascontiguousarray(nodes, np.uint32); idx = np.ascontiguousarray(prim_indices, np.uint32).ravel()
        b = np.ascontiguousarray(bounds, np.float32).ravel()
        assert nodes.ndim == 2 and b.shape[0] == 6
        fn = getattr(lib, "hprt_debug_%s_from_arrays" % cls._prefix)
        fn.restype = C.c_int
        fn.argtypes = [C.c_uint32] * len(head) + [C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_void_p)]
        h = C.c_void_p()
        _check(fn(*head, nodes.shape[0], _ptr(nodes), idx.shape[0], _ptr(idx), int(n_prims), _ptr(b), C.byref(h)))
        return cls(handle=h)

    def _directions(self):
        """[M, 3] float32: getDirections(M)"""
        d = np.zeros((self.info()["M"], 3), np.float32)
        self._call("copy", None, None, _ptr(d))
        return d

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:      # (module globals are cleared at interpreter exit)
            getattr(lib, "hprt_%s_destroy" % self._prefix)(self._h)
            self._h = None


class RbspKd(_Tree):
    """kd-aware RBSP tree (host): CreateRBSPKdTreeAccelerator(prims, params) — the RBSP node layout and direction table, with
    RBSPKd's cost model.  RbspKd(model) takes the scene's Accelerator line; keyword parameters override it."""
    _prefix = "rbspkd"
    _info_keys = ("nodes", "leaves", "prim_refs", "depth", "M", "kd_interior", "bsp_interior")

    def __init__(self, model=None, handle=None, n_directions=None, isect_cost=80, trav_cost=5, kd_trav_cost=1, empty_bonus=0.0, max_prims=1,
                 max_depth=-1, threads=0, device=None, min_candidates=0, max_edges=0, build_stats=None):
        """device: None builds on the host; a HIP device ordinal costs the split candidates of nodes with at least min_candidates
        candidates on that GPU (the same tree, byte for byte) and leaves HprtBuildDeviceStats as a dict in self.build_stats."""
        self.build_stats = build_stats
        if handle is None:
            prm = None if n_directions is None else C.byref(RbspKdParams(isect_cost, trav_cost, kd_trav_cost, empty_bonus, max_prims, max_depth,
                                                                           n_directions, threads))
            handle, self.build_stats = _build_tree("rbspkd", "build", (model._h,), prm, _device_opts(BuildDeviceOpts, device, min_candidates, max_edges))
        self._h = handle

    @staticmethod
    def from_triangles(p9, n_directions=3, isect_cost=80, trav_cost=5, kd_trav_cost=1, empty_bonus=0.0, max_prims=1, max_depth=-1, threads=0,
                       device=None, min_candidates=0, max_edges=0):
        """p9: [n, 9] (or [n, 3, 3]) float32 world-space triangle vertices in creation order.  device: as in the constructor."""
        p9 = np.ascontiguousarray(p9, np.float32).reshape(-1, 9)
        prm = RbspKdParams(isect_cost, trav_cost, kd_trav_cost, empty_bonus, max_prims, max_depth, n_directions, threads)
        h, st = _build_tree("rbspkd", "build_from_triangles", (p9.shape[0], _ptr(p9)), C.byref(prm),
                            _device_opts(BuildDeviceOpts, device, min_candidates, max_edges))
        return RbspKd(handle=h, build_stats=st)

    @staticmethod
    def from_arrays(nodes, prim_indices, n_prims, bounds, n_directions=3):
        """A tree made by hand (see _Tree._from_arrays); n_directions: 3, 7, 9 or 13, the library's own direction table."""
        return RbspKd._from_arrays(nodes, prim_indices, n_prims, bounds, n_directions)

    directions = _Tree._directions


class SceneDesc(C.Structure):
    _fields_ = [("nodes", C.c_void_p), ("n_nodes", C.c_uint32), ("prim_order", C.c_void_p), ("n_prims", C.c_uint32),
                ("shapes", C.POINTER(ShapeDesc)), ("n_shapes", C.c_uint32),
                ("materials", C.POINTER(MaterialDesc)), ("n_materials", C.c_uint32),
                ("lights", C.POINTER(LightDesc)), ("n_lights", C.c_uint32), ("light_strategy", C.c_int32),
                ("textures", C.c_void_p), ("n_textures", C.c_uint32),
                ("objects", C.c_void_p), ("n_objects", C.c_uint32), ("instances", C.c_void_p), ("n_instances", C.c_uint32),
                ("top", C.c_void_p), ("n_top", C.c_uint32)]


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError("hprt: %s is missing — run `python thesis-pbrt-v3_amd/build.py` (hipcc, gfx950). "
                          "There is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    vp, cp, i32, u32, u64, sz = C.c_void_p, C.c_char_p, C.c_int32, C.c_uint32, C.c_uint64, C.c_size_t
    P = C.POINTER
    sig = {
        "hprt_last_error": (cp, []),
        "hprt_version": (cp, []),
        "hprt_model_parse": (C.c_int, [cp, P(cp), C.c_int, P(vp)]),
        "hprt_model_load": (C.c_int, [cp, P(vp)]),
        "hprt_model_save": (C.c_int, [vp, cp]),
        "hprt_model_save_compact": (C.c_int, [vp, cp]),
        "hprt_model_destroy": (None, [vp]),
        "hprt_model_get_options": (C.c_int, [vp, P(RenderOptions)]),
        "hprt_model_set_options": (C.c_int, [vp, P(RenderOptions)]),
        "hprt_model_counts": (C.c_int, [vp, P(u64)]),
        "hprt_model_warnings": (cp, [vp]),
        "hprt_model_texture_info": (C.c_int, [vp, C.c_uint32, P(C.c_int32), P(C.c_float)]),
        "hprt_model_texture_level": (C.c_int, [vp, C.c_uint32, C.c_uint32, P(C.c_int32), vp]),
        "hprt_bvh_build": (C.c_int, [vp, P(vp)]),
        "hprt_bvh_build_from_bounds": (C.c_int, [sz, vp, vp, C.c_int, C.c_int, C.c_int, P(vp)]),
        "hprt_bvh_destroy": (None, [vp]),
        "hprt_bvh_info": (C.c_int, [vp, P(u32), P(C.c_float)]),
        "hprt_bvh_copy": (C.c_int, [vp, vp, vp]),
        "hprt_bvh_object_info": (C.c_int, [vp, C.c_uint32, P(u32), P(C.c_float)]),
        "hprt_bvh_object_copy": (C.c_int, [vp, C.c_uint32, vp, vp]),
        "hprt_bvhold_build": (C.c_int, [vp, vp, P(vp)]),
        "hprt_bvhold_build_from_bounds": (C.c_int, [sz, vp, vp, vp, P(vp)]),
        "hprt_bvhold_build_device": (C.c_int, [vp, vp, vp, vp, P(vp)]),
        "hprt_bvhold_build_device_from_bounds": (C.c_int, [sz, vp, vp, vp, vp, vp, P(vp)]),
        "hprt_scene_create": (C.c_int, [vp, C.c_int, P(vp)]),
        "hprt_scene_create_from_model": (C.c_int, [vp, vp, C.c_int, P(vp)]),
        "hprt_scene_destroy": (None, [vp]),
        "hprt_intersect": (C.c_int, [vp, sz, vp, vp, vp, vp, vp, vp, vp]),
        "hprt_occluded": (C.c_int, [vp, sz, vp, vp, vp, vp, vp]),
        "hprt_intersect_instanced": (C.c_int, [vp, sz, vp, vp, vp, vp, vp, vp, vp, vp]),
        "hprt_intersect_device": (C.c_int, [vp, sz, vp, vp, vp, vp, vp]),
        "hprt_occluded_device": (C.c_int, [vp, sz, vp, vp, vp]),
        "hprt_render": (C.c_int, [vp, P(RenderDesc), vp, vp, P(RenderStats)]),
        "hprt_film_resolve": (C.c_int, [vp, sz, C.c_float, vp]),
        "hprt_film_read": (C.c_int, [vp, vp, sz]),
        "hprt_pixel_stats_read": (C.c_int, [vp, vp, sz]),
        "hprt_write_pixel_stats": (C.c_int, [cp, vp, C.c_int, C.c_int]),
        "hprt_write_pfm": (C.c_int, [cp, vp, C.c_int, C.c_int]),
        "hprt_sample_radiance": (C.c_int, [vp, P(RenderOptions), sz, vp, vp, vp, vp]),
        "hprt_halton_permutations": (C.c_int, [vp, sz, P(sz)]),
        "hprt_comm_unique_id": (C.c_int, [vp]),
        "hprt_comm_create": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, P(vp)]),
        "hprt_comm_info": (C.c_int, [vp, P(C.c_int), P(C.c_int), P(C.c_int)]),
        "hprt_comm_destroy": (None, [vp]),
        "hprt_film_gather": (C.c_int, [vp, vp, vp, sz, C.c_int, vp]),
        "hprt_film_gather_local": (C.c_int, [P(vp), P(vp), C.c_int, sz, C.c_int]),
        "hprt_film_gather_local_shutdown": (None, []),
        "hprt_scene_reserve": (C.c_int, [vp, P(RenderDesc)]),
        "hprt_film_records_read": (C.c_int, [vp, vp, sz, P(sz)]),
        "hprt_film_records_merge": (C.c_int, [vp, sz, vp, sz]),
        "hprt_model_accelerator": (C.c_int, [vp, vp, sz]),
        "hprt_kdtree_build": (C.c_int, [vp, P(vp)]),
        "hprt_kdtree_build_from_bounds": (C.c_int, [sz, vp, vp, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, P(vp)]),
        "hprt_kdtree_info": (C.c_int, [vp, P(u32)]),
        "hprt_kdtree_copy": (C.c_int, [vp, vp, vp]),
        "hprt_kdtree_destroy": (None, [vp]),
        "hprt_scene_attach_kdtree": (C.c_int, [vp, vp]),
        "hprt_kdinst_build": (C.c_int, [vp, P(vp)]),
        "hprt_kdinst_info": (C.c_int, [vp, P(u32)]),
        "hprt_kdinst_object_info": (C.c_int, [vp, u32, P(u32)]),
        "hprt_kdinst_copy": (C.c_int, [vp, vp, vp]),
        "hprt_kdinst_object_copy": (C.c_int, [vp, u32, vp, vp]),
        "hprt_kdinst_destroy": (None, [vp]),
        "hprt_scene_attach_kdinst": (C.c_int, [vp, vp]),
        "hprt_write_pixel_stats_accel": (C.c_int, [cp, vp, C.c_int, C.c_int, C.c_int]),
        "hprt_rbsp_build": (C.c_int, [vp, vp, P(vp)]),
        "hprt_rbsp_build_from_triangles": (C.c_int, [sz, vp, vp, P(vp)]),
        "hprt_rbsp_info": (C.c_int, [vp, P(u32)]),
        "hprt_rbsp_copy": (C.c_int, [vp, vp, vp, vp]),
        "hprt_rbsp_destroy": (None, [vp]),
        "hprt_scene_attach_rbsp": (C.c_int, [vp, vp]),
        "hprt_rbspkd_build": (C.c_int, [vp, vp, P(vp)]),
        "hprt_rbspkd_build_from_triangles": (C.c_int, [sz, vp, vp, P(vp)]),
        "hprt_rbspkd_info": (C.c_int, [vp, P(u32)]),
        "hprt_rbspkd_copy": (C.c_int, [vp, vp, vp, vp]),
        "hprt_rbspkd_destroy": (None, [vp]),
        "hprt_scene_attach_rbspkd": (C.c_int, [vp, vp]),
        "hprt_rbspinst_build": (C.c_int, [vp, vp, P(vp)]),
        "hprt_rbspkdinst_build": (C.c_int, [vp, vp, P(vp)]),
        "hprt_rbspinst_info": (C.c_int, [vp, P(u32)]),
        "hprt_rbspinst_object_info": (C.c_int, [vp, u32, P(u32)]),
        "hprt_rbspinst_copy": (C.c_int, [vp, vp, vp, vp]),
        "hprt_rbspinst_object_copy": (C.c_int, [vp, u32, vp, vp]),
        "hprt_rbspinst_destroy": (None, [vp]),
        "hprt_scene_attach_rbspinst": (C.c_int, [vp, vp]),
        "hprt_rbsp_build_device": (C.c_int, [vp, vp, vp, vp, P(vp)]),
        "hprt_rbsp_build_from_triangles_device": (C.c_int, [sz, vp, vp, vp, vp, P(vp)]),
        "hprt_rbspkd_build_device": (C.c_int, [vp, vp, vp, vp, P(vp)]),
        "hprt_rbspkd_build_from_triangles_device": (C.c_int, [sz, vp, vp, vp, vp, P(vp)]),
        "hprt_bsppaper_build_device": (C.c_int, [vp, vp, vp, vp, P(vp)]),
        "hprt_bsppaper_build_from_triangles_device": (C.c_int, [sz, vp, vp, vp, vp, P(vp)]),
        "hprt_bsppaperkd_build_device": (C.c_int, [vp, vp, vp, vp, P(vp)]),
        "hprt_bsppaperkd_build_from_triangles_device": (C.c_int, [sz, vp, vp, vp, vp, P(vp)]),
        "hprt_bsppaper_build": (C.c_int, [vp, vp, P(vp)]),
        "hprt_bsppaper_build_from_triangles": (C.c_int, [sz, vp, vp, P(vp)]),
        "hprt_bsppaper_info": (C.c_int, [vp, P(u32)]),
        "hprt_bsppaper_copy": (C.c_int, [vp, vp, vp]),
        "hprt_bsppaper_destroy": (None, [vp]),
        "hprt_scene_attach_bsppaper": (C.c_int, [vp, vp]),
        "hprt_bsppaperkd_build": (C.c_int, [vp, vp, P(vp)]),
        "hprt_bsppaperkd_build_from_triangles": (C.c_int, [sz, vp, vp, P(vp)]),
        "hprt_bsppaperkd_info": (C.c_int, [vp, P(u32)]),
        "hprt_bsppaperkd_copy": (C.c_int, [vp, vp, vp]),
        "hprt_bsppaperkd_destroy": (None, [vp]),
        "hprt_scene_attach_bsppaperkd": (C.c_int, [vp, vp]),
        "hprt_bsppaperinst_build": (C.c_int, [vp, vp, P(vp)]),
        "hprt_bsppaperkdinst_build": (C.c_int, [vp, vp, P(vp)]),
        "hprt_bsppaperinst_info": (C.c_int, [vp, P(u32)]),
        "hprt_bsppaperinst_object_info": (C.c_int, [vp, u32, P(u32)]),
        "hprt_bsppaperinst_copy": (C.c_int, [vp, vp, vp]),
        "hprt_bsppaperinst_object_copy": (C.c_int, [vp, u32, vp, vp]),
        "hprt_bsppaperinst_destroy": (None, [vp]),
        "hprt_scene_attach_bsppaperinst": (C.c_int, [vp, vp]),
        "hprt_bspnode_build": (C.c_int, [vp, vp, P(vp)]),
        "hprt_bspnode_build_from_triangles": (C.c_int, [sz, vp, vp, P(vp)]),
        "hprt_bspnodekd_build": (C.c_int, [vp, vp, P(vp)]),
        "hprt_bspnodekd_build_from_triangles": (C.c_int, [sz, vp, vp, P(vp)]),
        "hprt_bspnode_build_device": (C.c_int, [vp, vp, vp, vp, P(vp)]),
        "hprt_bspnode_build_from_triangles_device": (C.c_int, [sz, vp, vp, vp, vp, P(vp)]),
        "hprt_bspnodekd_build_device": (C.c_int, [vp, vp, vp, vp, P(vp)]),
        "hprt_bspnodekd_build_from_triangles_device": (C.c_int, [sz, vp, vp, vp, vp, P(vp)]),
        "hprt_bspnodeinst_build": (C.c_int, [vp, vp, P(vp)]),
        "hprt_bspnodeinst_build_device": (C.c_int, [vp, vp, vp, vp, P(vp)]),
        "hprt_scene_kd_counters": (C.c_int, [vp, vp]),
        "hprt_pixel_kd_stats_read": (C.c_int, [vp, vp, sz]),
        "hprt_write_pixel_stats_rbspkd": (C.c_int, [cp, vp, vp, C.c_int, C.c_int]),
        "hprt_model_integrator": (C.c_int, [vp, vp, sz, P(AoParams)]),
        "hprt_render_ao": (C.c_int, [vp, P(RenderDesc), P(AoParams), vp, vp, P(RenderStats)]),
        "hprt_sample_ao": (C.c_int, [vp, P(RenderOptions), P(AoParams), sz, vp, vp, vp, vp]),
        "hprt_model_direct": (C.c_int, [vp, P(DirectParams), vp, sz, P(sz)]),
        "hprt_render_direct": (C.c_int, [vp, P(RenderDesc), P(DirectParams), vp, sz, vp, vp, P(RenderStats)]),
        "hprt_sample_direct": (C.c_int, [vp, P(RenderOptions), P(DirectParams), vp, sz, sz, vp, vp, vp, vp]),
    }
    # the two-level handles' diagnostics hooks (not part of include/hprt.h, so not among EXPORTS)
    debug = {}
    for prefix in ("kdinst", "rbspinst", "bsppaperinst"):
        debug["hprt_debug_%s_bounds" % prefix] = (C.c_int, [vp, C.c_int, vp])
        debug["hprt_debug_%s_set_tree" % prefix] = (C.c_int, [vp, C.c_int, sz, vp, sz, vp, vp])
    debug["hprt_debug_ao_ray_capacity"] = (sz, [sz])
    debug["hprt_debug_ao_kernel_seconds"] = (C.c_int, [vp, vp])
    debug["hprt_debug_dl_ray_capacity"] = (sz, [sz])
    debug["hprt_debug_dl_kernel_seconds"] = (C.c_int, [vp, vp])
    debug["hprt_debug_halton_index"] = (C.c_int, [P(RenderOptions), sz, vp, vp, vp, vp, vp, vp])
    # the light-centred shadow grid (csrc/shadow_grid.h)
    debug["hprt_debug_shadow_grid"] = (C.c_int, [C.c_int])
    debug["hprt_debug_shadow_grid_info"] = (C.c_int, [vp, vp])
    debug["hprt_debug_shadow_grid_occluded"] = (C.c_int, [vp, sz, vp, vp, vp])
    debug["hprt_debug_shadow_grid_build"] = (C.c_int, [sz, vp, vp, C.c_uint32, vp, vp, sz, vp, sz])
    debug["hprt_debug_shadow_grid_image"] = (C.c_int, [sz, vp, vp, C.c_uint32, vp, vp, sz, vp, sz])
    debug["hprt_debug_shadow_grid_image_read"] = (C.c_int, [vp, vp, vp, sz, vp, sz])
    # the light-aligned grid of a distant light (csrc/distant_grid.h)
    debug["hprt_debug_shadow_grid_layout"] = (C.c_int, [vp, vp, vp])
    debug["hprt_debug_distant_grid_info"] = (C.c_int, [vp, vp])
    debug["hprt_debug_distant_grid_occluded"] = (C.c_int, [vp, sz, vp, vp, vp])
    debug["hprt_debug_distant_grid_build"] = (C.c_int, [sz, vp, vp, vp, C.c_uint32, vp, vp, sz, vp, sz])
    debug["hprt_debug_distant_grid_image"] = (C.c_int, [sz, vp, vp, vp, C.c_uint32, vp, vp, sz, vp, sz])
    debug["hprt_debug_distant_grid_image_read"] = (C.c_int, [vp, vp, vp, sz, vp, sz])
    for name, (res, args) in list(sig.items()) + list(debug.items()):
        fn = getattr(lib, name)   # raises AttributeError if an export is missing
        fn.restype = res
        fn.argtypes = args
    return lib, sorted(sig)


lib, EXPORTS = _load()


def _check(rc):
    if rc != 0:
        raise HprtError(rc, lib.hprt_last_error().decode("utf-8", "replace"))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def version():
    return lib.hprt_version().decode()


_probe_lib = None


def _probe():
    """lib/libhprt_probe.so (build.py): the device probes of the tests, in a library of their own beside libhprt.so."""
    global _probe_lib
    if _probe_lib is None:
        path = os.path.join(os.path.dirname(LIB_PATH), "libhprt_probe.so")
        if not os.path.exists(path):
            raise ImportError("hprt: %s is missing — run `python thesis-pbrt-v3_amd/build.py`" % path)
        p = C.CDLL(path)
        p.hprt_debug_device_halton.restype = C.c_int
        p.hprt_debug_device_halton.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        p.hprt_debug_device_bsdf.restype = C.c_int
        p.hprt_debug_device_bsdf.argtypes = [C.c_void_p, C.c_int, C.c_size_t] + [C.c_void_p] * 6
        p.hprt_debug_device_bsdf_specular.restype = C.c_int
        p.hprt_debug_device_bsdf_specular.argtypes = [C.c_void_p, C.c_int, C.c_size_t] + [C.c_void_p] * 5
        _probe_lib = p
    return _probe_lib


SG_SINGLE, SG_PRIM_MASK = 0x80000000, 0x0fffffff


def debug_shadow_grid(on):
    """Test hook (not part of include/hprt.h): 0 sends the shadow rays of later plain renders through the walk, 1 through the light-centred
    grid where a scene has one, -1 back to the default (HPRT_SHADOW_GRID at scene creation); returns the setting before."""
    return lib.hprt_debug_shadow_grid(int(on))


def debug_ao_ray_capacity(rays):
    """Test hook (not part of include/hprt.h): the hemisphere rays one any-hit launch of later render_ao calls takes at most (never fewer
    than one hit's n_samples); 0: back to the default.  Returns the setting before."""
    return int(lib.hprt_debug_ao_ray_capacity(int(rays)))


def debug_dl_ray_capacity(items):
    """Test hook (not part of include/hprt.h): the light samples one pair of trace launches of later render_direct calls takes at most (never
    fewer than one hit's); 0: back to the default.  Returns the setting before."""
    return int(lib.hprt_debug_dl_ray_capacity(int(items)))


def shadow_grid_build(p9, light, res):
    """Test hook (not part of include/hprt.h; host only): the shadow grid of the triangles p9 ([n, 9] float32, each a leaf of its own)
    around the point `light` at res x res cells per cube face.  dict: R, eps, near (near-list length), longest, seconds, cell_start
    (uint32 [6 R^2 + 1]), prim (entry -> triangle), single (entry -> SG_SINGLE mark), key (entry -> float32 depth key), rect (entry ->
    [u0, u1, v0, v1], the sixteenths of its cell the triangle reaches, inclusive); the first `near` entries are the near list."""
    p9 = np.ascontiguousarray(p9, np.float32).reshape(-1, 9)
    light = np.ascontiguousarray(light, np.float32)
    info = np.zeros(6, np.float64)
    _check(lib.hprt_debug_shadow_grid_build(p9.shape[0], _ptr(p9), _ptr(light), int(res), _ptr(info), None, 0, None, 0))
    R, n_entries = int(info[0]), int(info[1])
    cell_start = np.zeros(6 * R * R + 1, np.uint32); entries = np.zeros((max(1, n_entries), 2), np.uint32)
    _check(lib.hprt_debug_shadow_grid_build(p9.shape[0], _ptr(p9), _ptr(light), int(res), _ptr(info), _ptr(cell_start), cell_start.size, _ptr(entries), entries.shape[0]))
    entries = entries[:n_entries]
    return {"R": R, "eps": float(info[3]), "near": int(info[2]), "longest": int(info[4]), "seconds": float(info[5]), "cell_start": cell_start,
            "prim": (entries[:, 0] & SG_PRIM_MASK).astype(np.int64), "single": (entries[:, 0] & SG_SINGLE) != 0, "key": (entries[:, 1] & np.uint32(0xffff0000)).view(np.float32),
            "rect": np.stack([(entries[:, 1] >> s) & 15 for s in (0, 4, 8, 12)], axis=1).astype(np.int64)}


SG_BLOCK_WORDS, SG_RECORD_WORDS, SG_BLOCK_SLOTS = 32, 12, 2
DG_DEFAULT_RES = 1024      # csrc/distant_grid.h


def shadow_grid_image_decode(blocks, records, R, near, faces=6):
    """The lists of a shadow grid's device image (csrc/shadow_grid.h, ShadowGridImage) as the kernel follows them: per cell the block's
    slots, then the run of records its head points to; before them the near list, records 0 .. near - 1.  faces: 6 for a point light's
    grid, 1 for a distant light's.  dict: blocks [faces R^2, 32] and
    records [n, 12] uint32, count (per cell), overflow (per cell: the record of its third entry), cell_start (int64 [faces R^2 + 1], the
    near list first, as ShadowGrid::cellStart), and per entry in list order prim_word, key_word (uint32), verts ([n, 9] uint32, the
    vertex floats' bits), next_key (uint32: the fourth lane of a record's third word; 0 for block slots), key2 (per cell: the block's
    copy of entry 2's key word)."""
    blocks = np.asarray(blocks, np.uint32).reshape(faces * R * R, SG_BLOCK_WORDS)
    records = np.asarray(records, np.uint32).reshape(-1, SG_RECORD_WORDS)
    count = blocks[:, 0].astype(np.int64); overflow = blocks[:, 1].astype(np.int64)
    cell_start = near + np.concatenate([[0], np.cumsum(count)])
    n = int(cell_start[-1])
    prim = np.zeros(n, np.uint32); key = np.zeros(n, np.uint32); nxt = np.zeros(n, np.uint32); verts = np.zeros((n, 9), np.uint32)
    vcols = [0, 1, 2, 4, 5, 6, 8, 9, 10]

    def from_records(dst, src):
        prim[dst] = records[src, 3]; key[dst] = records[src, 7]; nxt[dst] = records[src, 11]; verts[dst] = records[src][:, vcols]

    from_records(np.arange(near), np.arange(near))
    for slot, (pw, kw, v0) in enumerate([((0, 2), (0, 3), 4), ((0, 7), (0, 11), 16)]):
        cells = np.nonzero(count > slot)[0]
        dst = cell_start[cells] + slot
        prim[dst] = blocks[cells, pw[1]]; key[dst] = blocks[cells, kw[1]]
        verts[dst] = blocks[cells][:, [v0 + c for c in vcols]]
    over = np.maximum(count - SG_BLOCK_SLOTS, 0)
    cells = np.repeat(np.arange(count.size), over)
    k = np.arange(int(over.sum())) - np.repeat(np.cumsum(over) - over, over)      # 0, 1, .. within each run
    from_records(cell_start[cells] + SG_BLOCK_SLOTS + k, overflow[cells] + k)
    return {"blocks": blocks, "records": records, "count": count, "overflow": overflow, "cell_start": cell_start, "prim_word": prim, "key_word": key,
            "verts": verts, "next_key": nxt, "key2": blocks[:, 15]}


def shadow_grid_image(p9, light, res):
    """Test hook (not part of include/hprt.h; host only): the device image of the grid shadow_grid_build gives for the same arguments,
    decoded by shadow_grid_image_decode; "words": (block words, record words with the padding, the words ShadowGridImageBytes counts)."""
    p9 = np.ascontiguousarray(p9, np.float32).reshape(-1, 9)
    light = np.ascontiguousarray(light, np.float32)
    words = np.zeros(3, np.uint64)
    _check(lib.hprt_debug_shadow_grid_image(p9.shape[0], _ptr(p9), _ptr(light), int(res), _ptr(words), None, 0, None, 0))
    blocks = np.zeros(int(words[0]), np.uint32); records = np.zeros(int(words[1]), np.uint32)
    _check(lib.hprt_debug_shadow_grid_image(p9.shape[0], _ptr(p9), _ptr(light), int(res), _ptr(words), _ptr(blocks), blocks.size, _ptr(records), records.size))
    info = np.zeros(6, np.float64)
    _check(lib.hprt_debug_shadow_grid_build(p9.shape[0], _ptr(p9), _ptr(light), int(res), _ptr(info), None, 0, None, 0))
    out = shadow_grid_image_decode(blocks, records, int(res), int(info[2]))
    out["words"] = tuple(int(w) for w in words)
    return out


def _distant_grid_args(p9, direction, bound):
    p9 = np.ascontiguousarray(p9, np.float32).reshape(-1, 9)
    direction = np.ascontiguousarray(direction, np.float32)
    bound = None if bound is None else np.ascontiguousarray(bound, np.float32).reshape(6)
    return p9, direction, bound


def distant_grid_build(p9, direction, res, bound=None):
    """Test hook (not part of include/hprt.h; host only): the light-aligned shadow grid (csrc/distant_grid.h) of the triangles p9 ([n, 9]
    float32, each a leaf of its own) under a distant light in `direction` (towards the light, normalised in float32) at res x res
    cells, over `bound` ((min, max); None: the bound of the triangles).  dict as shadow_grid_build's, with cell_start uint32
    [R^2 + 1] (cell = iv * R + iu), margin and height_margin (world units), and the frame the device computes a ray's cell and key
    limit from: U, V, W (float32 [3]), u0, v0, scale_u, scale_v, h_top (float32)."""
    p9, direction, bound = _distant_grid_args(p9, direction, bound)
    info = np.zeros(22, np.float64)
    _check(lib.hprt_debug_distant_grid_build(p9.shape[0], _ptr(p9), _ptr(direction), _ptr(bound), int(res), _ptr(info), None, 0, None, 0))
    R, n_entries = int(info[0]), int(info[1])
    cell_start = np.zeros(R * R + 1, np.uint32); entries = np.zeros((max(1, n_entries), 2), np.uint32)
    _check(lib.hprt_debug_distant_grid_build(p9.shape[0], _ptr(p9), _ptr(direction), _ptr(bound), int(res), _ptr(info), _ptr(cell_start), cell_start.size, _ptr(entries), entries.shape[0]))
    entries = entries[:n_entries]
    f32 = np.float32
    return {"R": R, "eps": float(info[3]), "near": int(info[2]), "longest": int(info[4]), "seconds": float(info[5]), "margin": float(info[6]), "height_margin": float(info[7]),
            "U": info[8:11].astype(f32), "V": info[11:14].astype(f32), "W": info[14:17].astype(f32), "u0": f32(info[17]), "v0": f32(info[18]),
            "scale_u": f32(info[19]), "scale_v": f32(info[20]), "h_top": f32(info[21]), "cell_start": cell_start,
            "prim": (entries[:, 0] & SG_PRIM_MASK).astype(np.int64), "single": (entries[:, 0] & SG_SINGLE) != 0, "key": (entries[:, 1] & np.uint32(0xffff0000)).view(np.float32),
            "rect": np.stack([(entries[:, 1] >> s) & 15 for s in (0, 4, 8, 12)], axis=1).astype(np.int64)}


def shadow_grid_layout(model, bvh):
    """Test hook (not part of include/hprt.h; host only): which shadow grid the layout of Scene(model, bvh) holds, as HPRT_SHADOW_GRID,
    HPRT_SHADOW_GRID_RES and HPRT_SHADOW_GRID_MAX_MB stand.  dict: point (eligible, R), distant (eligible, R, entries, near, bytes, longest)."""
    out = np.zeros(8, np.float64)
    _check(lib.hprt_debug_shadow_grid_layout(model._h, bvh._h, _ptr(out)))
    return {"point": {"eligible": bool(out[0]), "R": int(out[1])},
            "distant": {"eligible": bool(out[2]), "R": int(out[3]), "entries": int(out[4]), "near": int(out[5]), "bytes": int(out[6]), "longest": int(out[7])}}


def distant_grid_image(p9, direction, res, bound=None):
    """Test hook (not part of include/hprt.h; host only): the device image of the grid distant_grid_build gives for the same arguments,
    decoded by shadow_grid_image_decode (faces = 1); "words" as shadow_grid_image's."""
    p9, direction, bound = _distant_grid_args(p9, direction, bound)
    words = np.zeros(3, np.uint64)
    _check(lib.hprt_debug_distant_grid_image(p9.shape[0], _ptr(p9), _ptr(direction), _ptr(bound), int(res), _ptr(words), None, 0, None, 0))
    blocks = np.zeros(int(words[0]), np.uint32); records = np.zeros(int(words[1]), np.uint32)
    _check(lib.hprt_debug_distant_grid_image(p9.shape[0], _ptr(p9), _ptr(direction), _ptr(bound), int(res), _ptr(words), _ptr(blocks), blocks.size, _ptr(records), records.size))
    info = np.zeros(22, np.float64)
    _check(lib.hprt_debug_distant_grid_build(p9.shape[0], _ptr(p9), _ptr(direction), _ptr(bound), int(res), _ptr(info), None, 0, None, 0))
    out = shadow_grid_image_decode(blocks, records, int(res), int(info[2]), faces=1)
    out["words"] = tuple(int(w) for w in words)
    return out


def debug_halton_index(opt, px, py, sample):
    """Test hook (not part of include/hprt.h; host only): the Halton indices of samples `sample` at pixels (px, py) of the frame `opt`
    describes, as a render forms them (SetupFrame's offset tables) and as sample_radiance does (HaltonPixelOffset), both uint64
    arrays, and the frame's sample bounds (sx0, sy0, sx1, sy1)."""
    px = np.ascontiguousarray(px, np.int32); py = np.ascontiguousarray(py, np.int32); sample = np.ascontiguousarray(sample, np.int64)
    a = np.zeros(px.shape[0], np.uint64); b = np.zeros(px.shape[0], np.uint64); bounds = np.zeros(4, np.int32)
    _check(lib.hprt_debug_halton_index(C.byref(opt), px.shape[0], _ptr(px), _ptr(py), _ptr(sample), _ptr(a), _ptr(b), _ptr(bounds)))
    return a, b, tuple(int(v) for v in bounds)


class Model:
    """Parsed scene (host)."""

    def __init__(self, handle):
        self._h = handle

    @staticmethod
    def parse(path, subst=None):
        kv = []
        for k, v in (subst or {}).items():
            kv += [k.encode(), v.encode()]
        arr = (C.c_char_p * max(1, len(kv)))(*kv)
        h = C.c_void_p()
        _check(lib.hprt_model_parse(path.encode(), arr, len(kv) // 2, C.byref(h)))
        return Model(h)

    @staticmethod
    def load(path):
        h = C.c_void_p()
        _check(lib.hprt_model_load(path.encode(), C.byref(h)))
        return Model(h)

    def save(self, path, compact=False):
        """Baked container; compact=True stores image textures as their source images (rebuilt at load) instead of float pyramids."""
        _check((lib.hprt_model_save_compact if compact else lib.hprt_model_save)(self._h, path.encode()))

    @property
    def options(self):
        o = RenderOptions()
        _check(lib.hprt_model_get_options(self._h, C.byref(o)))
        return o

    @options.setter
    def options(self, o):
        _check(lib.hprt_model_set_options(self._h, C.byref(o)))

    def counts(self):
        c = (C.c_uint64 * 7)()
        _check(lib.hprt_model_counts(self._h, c))
        return dict(zip(("shapes", "primitives", "triangles", "spheres", "materials", "lights", "textures"), [int(x) for x in c]))

    def texture(self, index):
        """Built MIPMap of image texture `index`: (info dict, [level arrays of shape (h, w, 3)], level 0 first, row 0 = t 0)."""
        info = (C.c_int32 * 5)(); ma = C.c_float()
        _check(lib.hprt_model_texture_info(self._h, index, info, C.byref(ma)))
        levels = []
        for k in range(info[0]):
            wh = (C.c_int32 * 2)()
            _check(lib.hprt_model_texture_level(self._h, index, k, wh, None))
            a = np.zeros((wh[1], wh[0], 3), np.float32)
            _check(lib.hprt_model_texture_level(self._h, index, k, wh, _ptr(a)))
            levels.append(a)
        return {"levels": info[0], "trilinear": bool(info[1]), "wrap": info[2], "max_anisotropy": ma.value}, levels

    @property
    def accelerator(self):
        """The scene's Accelerator name ("bvh", "kdtree", ...); baked models report "bvh"."""
        buf = C.create_string_buffer(256)
        _check(lib.hprt_model_accelerator(self._h, buf, 256))
        return buf.value.decode()

    def integrator(self):
        """(name, n_samples, cos_sample): the scene's Integrator name ("path", "ambientocclusion", ...) and the parameters of an
        "ambientocclusion" line (the defaults 64, True for any other name); baked models report "path"."""
        buf = C.create_string_buffer(256)
        ao = AoParams()
        _check(lib.hprt_model_integrator(self._h, buf, 256, C.byref(ao)))
        return buf.value.decode(), int(ao.n_samples), bool(ao.cos_sample)

    def direct(self):
        """(strategy, max_depth, n_light_samples): the parameters of the scene's Integrator "directlighting" line ("all" or "one", maxdepth;
        the defaults "all", 5 for any other name) and Light::nSamples of every scene light in scene.lights order, one per triangle of a
        mesh emitter; baked models report the defaults and 1 for every light."""
        dp = DirectParams()
        n = C.c_size_t(0)
        _check(lib.hprt_model_direct(self._h, C.byref(dp), None, 0, C.byref(n)))
        counts = np.zeros(max(1, n.value), np.int32)
        _check(lib.hprt_model_direct(self._h, None, _ptr(counts), n.value, None))
        return ("one" if dp.strategy == 1 else "all"), int(dp.max_depth), [int(v) for v in counts[:n.value]]

    def warnings(self):
        w = lib.hprt_model_warnings(self._h).decode()
        return [x for x in w.split("\n") if x]

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:      # (module globals are cleared at interpreter exit)
            lib.hprt_model_destroy(self._h)
            self._h = None


class Bvh:
    """Flattened BVH (host): CreateBVHAccelerator(prims, params)."""

    def __init__(self, model=None, handle=None):
        if handle is None:
            handle = C.c_void_p()
            _check(lib.hprt_bvh_build(model._h, C.byref(handle)))
        self._h = handle

    @staticmethod
    def from_bounds(bmin, bmax, max_node_prims=4, isect_cost=8, trav_cost=1):
        bmin = np.ascontiguousarray(bmin, np.float32); bmax = np.ascontiguousarray(bmax, np.float32)
        h = C.c_void_p()
        _check(lib.hprt_bvh_build_from_bounds(bmin.shape[0], _ptr(bmin), _ptr(bmax), max_node_prims, isect_cost, trav_cost, C.byref(h)))
        return Bvh(handle=h)

    def info(self):
        i = (C.c_uint32 * 4)()
        b = (C.c_float * 6)()
        _check(lib.hprt_bvh_info(self._h, i, b))
        return {"nodes": i[0], "prims": i[1], "leaves": i[2], "max_depth": i[3], "bounds": [float(x) for x in b]}

    def arrays(self):
        inf = self.info()
        nodes = np.zeros((inf["nodes"], 8), np.uint32)
        order = np.zeros(inf["prims"], np.uint32)
        _check(lib.hprt_bvh_copy(self._h, _ptr(nodes), _ptr(order)))
        return nodes, order

    def object_arrays(self, obj):
        """(nodes, prim_order) of the aggregate of object definition `obj` (core/api.cpp:1798-1806)."""
        i = (C.c_uint32 * 4)()
        _check(lib.hprt_bvh_object_info(self._h, obj, i, None))
        nodes = np.zeros((i[0], 8), np.uint32)
        order = np.zeros(i[1], np.uint32)
        _check(lib.hprt_bvh_object_copy(self._h, obj, _ptr(nodes), _ptr(order)))
        return nodes, order

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:      # (module globals are cleared at interpreter exit)
            lib.hprt_bvh_destroy(self._h)
            self._h = None


class BvhOldParams(C.Structure):
    """HprtBvhOldParams: CreateBVHAcceleratorOld's parameters."""
    _fields_ = [("split_method", C.c_int32), ("max_node_prims", C.c_int32)]


class BvhOldDeviceOpts(C.Structure):
    """HprtBvhOldDeviceOpts: the device build of the HLBVH form (0 = default)."""
    _fields_ = [("device", C.c_int), ("serial_treelet_max", C.c_uint32)]


class BvhOldDeviceStats(C.Structure):
    """HprtBvhOldDeviceStats"""
    _fields_ = [("prims_sorted", C.c_uint64), ("sort_passes", C.c_uint64), ("treelets", C.c_uint64), ("treelets_host", C.c_uint64),
                ("launches", C.c_uint64), ("seconds_device", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


BVHOLD_SPLIT_METHODS = {"sah": 0, "hlbvh": 1, "middle": 2, "equal": 3}      # HPRT_BVHOLD_*


class BvhOld(Bvh):
    """The stock pbrt-v3 BVH (host), Accelerator "bvhold": CreateBVHAcceleratorOld(prims, params).  An ordinary Bvh: Scene(model, BvhOld(model))
    walks it.  BvhOld(model) takes the scene's Accelerator line; split_method ("sah", "hlbvh", "middle", "equal") and max_node_prims
    override it (the other one then takes its default, "sah" or 4)."""

    def __init__(self, model=None, split_method=None, max_node_prims=None, device=None, serial_treelet_max=0, handle=None, build_stats=None):
        """device: None builds on the host; a HIP device ordinal builds the "hlbvh" form on that GPU (the same tree, byte for byte) and
        leaves HprtBvhOldDeviceStats as a dict in self.build_stats.  serial_treelet_max: treelets of more primitives are emitted on the host."""
        self.build_stats = build_stats
        if handle is None:
            handle, self.build_stats = BvhOld._build("build", (model._h,), split_method, max_node_prims, device, serial_treelet_max)
        self._h = handle

    @staticmethod
    def _build(how, head, split_method, max_node_prims, device, serial_treelet_max):
        prm = None
        if split_method is not None or max_node_prims is not None:
            sm = BVHOLD_SPLIT_METHODS[split_method] if isinstance(split_method, str) else (0 if split_method is None else int(split_method))
            prm = C.byref(BvhOldParams(sm, 4 if max_node_prims is None else int(max_node_prims)))
        h = C.c_void_p()
        if device is None:
            _check(getattr(lib, "hprt_bvhold_" + how)(*head, prm, C.byref(h)))
            return h, None
        opts, st = BvhOldDeviceOpts(int(device), int(serial_treelet_max)), BvhOldDeviceStats()
        dev_name = "hprt_bvhold_build_device" + how[len("build"):]
        _check(getattr(lib, dev_name)(*head, prm, C.byref(opts), C.byref(st), C.byref(h)))
        return h, st.as_dict()

    @staticmethod
    def from_bounds(bmin, bmax, split_method="sah", max_node_prims=4, device=None, serial_treelet_max=0):
        """bmin, bmax: [n, 3] float32 world bounds in creation order.  device: as in the constructor."""
        bmin = np.ascontiguousarray(bmin, np.float32).reshape(-1, 3); bmax = np.ascontiguousarray(bmax, np.float32).reshape(-1, 3)
        h, st = BvhOld._build("build_from_bounds", (bmin.shape[0], _ptr(bmin), _ptr(bmax)), split_method, max_node_prims, device, serial_treelet_max)
        return BvhOld(handle=h, build_stats=st)


class KdTree(_Tree):
    """kd-tree (host): CreateKdTreeAccelerator(prims, params) — KdAccelNode[] and primitiveIndices as the reference builds them."""
    _prefix = "kdtree"
    _info_keys = ("nodes", "leaves", "prim_refs", "depth")

    def __init__(self, model=None, handle=None):
        if handle is None:
            handle = C.c_void_p()
            _check(lib.hprt_kdtree_build(model._h, C.byref(handle)))
        self._h = handle

    @staticmethod
    def from_bounds(bmin, bmax, isect_cost=80, trav_cost=1, empty_bonus=0.0, max_prims=1, max_depth=-1):
        bmin = np.ascontiguousarray(bmin, np.float32); bmax = np.ascontiguousarray(bmax, np.float32)
        h = C.c_void_p()
        _check(lib.hprt_kdtree_build_from_bounds(bmin.shape[0], _ptr(bmin), _ptr(bmax), isect_cost, trav_cost, C.c_float(empty_bonus),
                                                 max_prims, max_depth, C.byref(h)))
        return KdTree(handle=h)

    @staticmethod
    def from_arrays(nodes, prim_indices, n_prims, bounds):
        """A tree made by hand (see _Tree._from_arrays)."""
        return KdTree._from_arrays(nodes, prim_indices, n_prims, bounds)


class _TwoLevel:
    """Two-level trees (host) of a model WITH object instances (KdInst, RbspInst, BspPaperInst) over the C calls hprt_<_prefix>_info /
    _object_info / _copy / _object_copy / _destroy and the diagnostics hooks hprt_debug_<_prefix>_bounds / _set_tree; info() names
    the words after the eight every handle has `_extra_keys`, and the copy of the RBSP trees takes a direction table as well.
    `_node_words`: the uint32 words of a node in copy() / object_copy() / set_tree() — 2, or the general BSP trees' 5."""
    _prefix = None
    _extra_keys = ()
    _node_words = 2
    _KEYS = ("nodes", "leaves", "prim_refs", "depth")

    def _fn(self, name, debug=False):
        return getattr(lib, "hprt_%s%s_%s" % ("debug_" if debug else "", self._prefix, name))

    def info(self):
        """the top-level tree's nodes, leaves, prim_refs and depth; objects (definitions), object_trees (those with more than one
        primitive), object_depth (the deepest object tree's) and instances; RbspInst: M (directions of every tree) and kd_aware;
        BspPaperInst: kd_aware, axis_interior (kd-aware: kd interior nodes) and plane_interior over all trees, reserved (0)"""
        keys = self._KEYS + ("objects", "object_trees", "object_depth", "instances") + self._extra_keys
        i = (C.c_uint32 * len(keys))()
        _check(self._fn("info")(self._h, i))
        return dict(zip(keys, i))

    def object_info(self, obj):
        """nodes, leaves, prim_refs and depth of the tree of object definition `obj`: all zero for an object of one primitive"""
        i = (C.c_uint32 * 4)()
        _check(self._fn("object_info")(self._h, obj, i))
        return dict(zip(self._KEYS, i))

    def copy(self):
        """(nodes [n, 2] uint32, prim_indices uint32) of the top-level tree, as KdTree.arrays() / Rbsp.arrays() give them
        (BspPaperInst: nodes [n, 5], as BspPaper.arrays() / BspPaperKd.arrays())"""
        inf = self.info()
        nodes = np.zeros((inf["nodes"], self._node_words), np.uint32); idx = np.zeros(inf["prim_refs"], np.uint32)
        _check(self._fn("copy")(self._h, _ptr(nodes), _ptr(idx), *([None] if "M" in inf else [])))
        return nodes, idx

    def object_copy(self, obj):
        """the same for the tree of object definition `obj` (empty arrays for an object of one primitive)"""
        inf = self.object_info(obj)
        nodes = np.zeros((inf["nodes"], self._node_words), np.uint32); idx = np.zeros(inf["prim_refs"], np.uint32)
        _check(self._fn("object_copy")(self._h, obj, _ptr(nodes), _ptr(idx)))
        return nodes, idx

    def bounds(self, obj=-1):
        """Diagnostics hook (not part of include/hprt.h): the six floats pMin, pMax of the top-level tree (obj < 0) or of one
        object's tree."""
        b = np.zeros(6, np.float32)
        _check(self._fn("bounds", debug=True)(self._h, int(obj), _ptr(b)))
        return b

    def set_tree(self, obj, nodes, prim_indices, bounds):
        """Diagnostics hook (not part of include/hprt.h): a tree made by hand in place of the top-level tree (obj < 0) or of one
        object's tree — for an RbspInst over the handle's M directions; it passes the checks a built handle passes (HprtError
        E_INVALID / E_UNSUPPORTED, the handle unchanged)."""
        nodes = np.ascontiguousarray(nodes, np.uint32); idx = np.ascontiguousarray(prim_indices, np.uint32).ravel()
        b = np.ascontiguousarray(bounds, np.float32).ravel()
        assert nodes.ndim == 2 and nodes.shape[1] == self._node_words and b.shape[0] == 6
        _check(self._fn("set_tree", debug=True)(self._h, int(obj), nodes.shape[0], _ptr(nodes), idx.shape[0], _ptr(idx), _ptr(b)))

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:      # (module globals are cleared at interpreter exit)
            self._fn("destroy")(self._h)
            self._h = None


class KdInst(_TwoLevel):
    """Two-level kd-trees (host) of a model WITH object instances, as pbrtObjectInstance and pbrtWorldEnd build them under
    Accelerator "kdtree" (core/api.cpp:1794-1819): one kd-tree per object of more than one primitive and the top-level kd-tree
    over the top-level items, all with the parameters of the scene's Accelerator line.  Scene.attach_kdinst walks them."""
    _prefix = "kdinst"

    def __init__(self, model):
        h = C.c_void_p()
        _check(lib.hprt_kdinst_build(model._h, C.byref(h)))
        self._h = h


class RbspParams(C.Structure):
    """HprtRbspParams: CreateRBSPTreeAccelerator's parameters plus the builder's thread count."""
    _fields_ = [("isect_cost", C.c_int), ("trav_cost", C.c_int), ("empty_bonus", C.c_float), ("max_prims", C.c_int),
                ("max_depth", C.c_int), ("n_directions", C.c_int), ("threads", C.c_int)]


def _rbsp_params(n_directions, isect_cost, trav_cost, empty_bonus, max_prims, max_depth, threads):
    return RbspParams(isect_cost, trav_cost, empty_bonus, max_prims, max_depth, n_directions, threads)


class Rbsp(_Tree):
    """RBSP tree (host): CreateRBSPTreeAccelerator(prims, params) — RBSPNode[], primitiveIndices and the direction table as
    the reference builds them.  Rbsp(model) takes the scene's Accelerator line; keyword parameters override it."""
    _prefix = "rbsp"
    _info_keys = ("nodes", "leaves", "prim_refs", "depth", "M")

    def __init__(self, model=None, handle=None, n_directions=None, isect_cost=80, trav_cost=5, empty_bonus=0.0, max_prims=1, max_depth=-1,
                 threads=0, device=None, min_candidates=0, max_edges=0, build_stats=None):
        """device: None builds on the host; a HIP device ordinal costs the split candidates of nodes with at least min_candidates
        candidates on that GPU (the same tree, byte for byte) and leaves HprtBuildDeviceStats as a dict in self.build_stats."""
        self.build_stats = build_stats
        if handle is None:
            prm = None if n_directions is None else C.byref(_rbsp_params(n_directions, isect_cost, trav_cost, empty_bonus, max_prims, max_depth, threads))
            handle, self.build_stats = _build_tree("rbsp", "build", (model._h,), prm, _device_opts(BuildDeviceOpts, device, min_candidates, max_edges))
        self._h = handle

    @staticmethod
    def from_triangles(p9, n_directions=3, isect_cost=80, trav_cost=5, empty_bonus=0.0, max_prims=1, max_depth=-1, threads=0,
                       device=None, min_candidates=0, max_edges=0):
        """p9: [n, 9] (or [n, 3, 3]) float32 world-space triangle vertices in creation order.  device: as in the constructor."""
        p9 = np.ascontiguousarray(p9, np.float32).reshape(-1, 9)
        prm = _rbsp_params(n_directions, isect_cost, trav_cost, empty_bonus, max_prims, max_depth, threads)
        h, st = _build_tree("rbsp", "build_from_triangles", (p9.shape[0], _ptr(p9)), C.byref(prm),
                            _device_opts(BuildDeviceOpts, device, min_candidates, max_edges))
        return Rbsp(handle=h, build_stats=st)

    @staticmethod
    def from_arrays(nodes, prim_indices, n_prims, bounds, n_directions=3):
        """A tree made by hand (see _Tree._from_arrays); n_directions: 3, 7, 9 or 13, the library's own direction table."""
        return Rbsp._from_arrays(nodes, prim_indices, n_prims, bounds, n_directions)

    directions = _Tree._directions


class RbspInst(_TwoLevel):
    """Two-level RBSP trees (host) of a model WITH object instances, as pbrtObjectInstance and pbrtWorldEnd build them under
    Accelerator "rbsp" — or, with kd_aware, "rbspkd" — (core/api.cpp:1794-1819): one tree per object of more than one primitive
    and the top-level tree over the top-level items, all with the same parameters.  RbspInst(model) takes the scene's Accelerator
    line; giving n_directions makes the keyword parameters replace it, as for Rbsp / RbspKd.  Scene.attach_rbspinst walks them."""
    _prefix = "rbspinst"
    _extra_keys = ("M", "kd_aware")

    def __init__(self, model, kd_aware=False, n_directions=None, isect_cost=80, trav_cost=5, kd_trav_cost=1, empty_bonus=0.0, max_prims=1,
                 max_depth=-1, threads=0):
        h = C.c_void_p()
        if kd_aware:
            prm = None if n_directions is None else C.byref(RbspKdParams(isect_cost, trav_cost, kd_trav_cost, empty_bonus, max_prims, max_depth,
                                                                           n_directions, threads))
            _check(lib.hprt_rbspkdinst_build(model._h, prm, C.byref(h)))
        else:
            prm = None if n_directions is None else C.byref(_rbsp_params(n_directions, isect_cost, trav_cost, empty_bonus, max_prims, max_depth, threads))
            _check(lib.hprt_rbspinst_build(model._h, prm, C.byref(h)))
        self._h = h

    def directions(self):
        """[M, 3] float32: getDirections(M), the one table of every tree"""
        d = np.zeros((self.info()["M"], 3), np.float32)
        _check(lib.hprt_rbspinst_copy(self._h, None, None, _ptr(d)))
        return d


class BspPaperParams(C.Structure):
    """HprtBspPaperParams: CreateBSPPaperTreeAccelerator's parameters plus the builder's thread count."""
    _fields_ = [("isect_cost", C.c_int), ("trav_cost", C.c_int), ("empty_bonus", C.c_float), ("max_prims", C.c_int),
                ("max_depth", C.c_int), ("threads", C.c_int)]


class BspPaper(_Tree):
    """General BSP tree (host): CreateBSPPaperTreeAccelerator(prims, params) — BSPNode[] (20 bytes: flags word pair and split
    axis) and primitiveIndices as the reference builds them.  BspPaper(model) takes the scene's Accelerator line; given
    isect_cost, the keyword parameters replace it (as n_directions does for Rbsp)."""
    _prefix = "bsppaper"
    _info_keys = ("nodes", "leaves", "depth", "prim_refs", "axis_interior", "plane_interior")

    def __init__(self, model=None, handle=None, isect_cost=None, trav_cost=5, empty_bonus=0.0, max_prims=1, max_depth=-1, threads=0, device=None, min_candidates=0, max_edges=0, max_faces=0,
                 max_face_edges=0, max_stack=0, build_stats=None):
        """device: None builds on the host; a HIP device ordinal costs the split candidates of nodes with at least min_candidates
        candidates on that GPU (the same tree, byte for byte) and leaves HprtBuildDeviceStats as a dict in self.build_stats.
        max_edges / max_faces / max_face_edges / max_stack: 0, or a value that lowers the kernel's compiled capacity."""
        self.build_stats = build_stats
        if handle is None:
            prm = None if isect_cost is None else C.byref(BspPaperParams(isect_cost, trav_cost, empty_bonus, max_prims, max_depth, threads))
            handle, self.build_stats = _build_tree("bsppaper", "build", (model._h,), prm,
                                                   _device_opts(BspBuildDeviceOpts, device, min_candidates, max_edges, max_faces, max_face_edges, max_stack))
        self._h = handle

    @staticmethod
    def from_triangles(p9, isect_cost=80, trav_cost=5, empty_bonus=0.0, max_prims=1, max_depth=-1, threads=0, device=None, min_candidates=0,
                       max_edges=0, max_faces=0, max_face_edges=0, max_stack=0):
        """p9: [n, 9] (or [n, 3, 3]) float32 world-space triangle vertices in creation order.  device ...: as in the constructor."""
        p9 = np.ascontiguousarray(p9, np.float32).reshape(-1, 9)
        prm = BspPaperParams(isect_cost, trav_cost, empty_bonus, max_prims, max_depth, threads)
        h, st = _build_tree("bsppaper", "build_from_triangles", (p9.shape[0], _ptr(p9)), C.byref(prm),
                            _device_opts(BspBuildDeviceOpts, device, min_candidates, max_edges, max_faces, max_face_edges, max_stack))
        return BspPaper(handle=h, build_stats=st)

    @staticmethod
    def from_arrays(nodes, prim_indices, n_prims, bounds):
        """A tree made by hand (see _Tree._from_arrays)."""
        return BspPaper._from_arrays(nodes, prim_indices, n_prims, bounds)

    def arrays(self):
        """(nodes [n, 5] uint32: the reference's BSPNode — word 0 split / onePrimitive / primitiveIndicesOffset, word 1 flags,
        words 2-4 splitAxis as float bits (zero for leaves); prim_indices uint32)"""
        inf = self.info()
        nodes = np.zeros((inf["nodes"], 5), np.uint32)
        idx = np.zeros(inf["prim_refs"], np.uint32)
        self._call("copy", _ptr(nodes), _ptr(idx))
        return nodes, idx


class BspPaperKdParams(C.Structure):
    """HprtBspPaperKdParams: CreateBSPPaperKdTreeAccelerator's parameters plus the builder's thread count."""
    _fields_ = [("isect_cost", C.c_int), ("trav_cost", C.c_int), ("kd_trav_cost", C.c_int), ("empty_bonus", C.c_float), ("max_prims", C.c_int),
                ("max_depth", C.c_int), ("threads", C.c_int)]


class BspPaperKd(_Tree):
    """kd-aware general BSP tree (host): CreateBSPPaperKdTreeAccelerator(prims, params) — BSPKdNode[] (20 bytes) and
    primitiveIndices as the reference builds them.  BspPaperKd(model) takes the scene's Accelerator line; given isect_cost, the
    keyword parameters replace it."""
    _prefix = "bsppaperkd"
    _info_keys = ("nodes", "leaves", "depth", "prim_refs", "kd_interior", "plane_interior")

    def __init__(self, model=None, handle=None, isect_cost=None, trav_cost=5, kd_trav_cost=1, empty_bonus=0.0, max_prims=1, max_depth=-1, threads=0, device=None, min_candidates=0, max_edges=0, max_faces=0,
                 max_face_edges=0, max_stack=0, build_stats=None):
        """device: None builds on the host; a HIP device ordinal costs the split candidates of nodes with at least min_candidates
        candidates on that GPU (the same tree, byte for byte) and leaves HprtBuildDeviceStats as a dict in self.build_stats.
        max_edges / max_faces / max_face_edges / max_stack: 0, or a value that lowers the kernel's compiled capacity."""
        self.build_stats = build_stats
        if handle is None:
            prm = None if isect_cost is None else C.byref(BspPaperKdParams(isect_cost, trav_cost, kd_trav_cost, empty_bonus, max_prims, max_depth, threads))
            handle, self.build_stats = _build_tree("bsppaperkd", "build", (model._h,), prm,
                                                   _device_opts(BspBuildDeviceOpts, device, min_candidates, max_edges, max_faces, max_face_edges, max_stack))
        self._h = handle

    @staticmethod
    def from_triangles(p9, isect_cost=80, trav_cost=5, kd_trav_cost=1, empty_bonus=0.0, max_prims=1, max_depth=-1, threads=0, device=None,
                       min_candidates=0, max_edges=0, max_faces=0, max_face_edges=0, max_stack=0):
        """p9: [n, 9] (or [n, 3, 3]) float32 world-space triangle vertices in creation order.  device ...: as in the constructor."""
        p9 = np.ascontiguousarray(p9, np.float32).reshape(-1, 9)
        prm = BspPaperKdParams(isect_cost, trav_cost, kd_trav_cost, empty_bonus, max_prims, max_depth, threads)
        h, st = _build_tree("bsppaperkd", "build_from_triangles", (p9.shape[0], _ptr(p9)), C.byref(prm),
                            _device_opts(BspBuildDeviceOpts, device, min_candidates, max_edges, max_faces, max_face_edges, max_stack))
        return BspPaperKd(handle=h, build_stats=st)

    @staticmethod
    def from_arrays(nodes, prim_indices, n_prims, bounds):
        """A tree made by hand (see _Tree._from_arrays)."""
        return BspPaperKd._from_arrays(nodes, prim_indices, n_prims, bounds)

    def arrays(self):
        """(nodes [n, 5] uint32: the reference's BSPKdNode — word 0 split / onePrimitive / primitiveIndicesOffset, word 1 flags
        (low 3 bits: 0-2 kd axis, 3 leaf, 4 plane node; aboveChild / nPrims << 3), words 2-4 splitAxis as float bits (zero for kd
        nodes and leaves); prim_indices uint32)"""
        inf = self.info()
        nodes = np.zeros((inf["nodes"], 5), np.uint32)
        idx = np.zeros(inf["prim_refs"], np.uint32)
        self._call("copy", _ptr(nodes), _ptr(idx))
        return nodes, idx


class BspPaperInst(_TwoLevel):
    """Two-level general BSP trees (host) of a model WITH object instances, as pbrtObjectInstance and pbrtWorldEnd build them under
    Accelerator "bsppaper" — or, with kd_aware, "bsppaperkd" — (core/api.cpp:1794-1819): one tree per object of more than one
    primitive and the top-level tree over the top-level items, all with the same parameters.  BspPaperInst(model) takes the scene's
    Accelerator line; given isect_cost, the keyword parameters replace it, as for BspPaper / BspPaperKd.  copy() / object_copy()
    return, and set_tree takes, the 5-word nodes of BspPaper.arrays() / BspPaperKd.arrays().  Scene.attach_bsppaperinst walks them."""
    _prefix = "bsppaperinst"
    _extra_keys = ("kd_aware", "axis_interior", "plane_interior", "reserved")
    _node_words = 5

    def __init__(self, model, kd_aware=False, isect_cost=None, trav_cost=5, kd_trav_cost=1, empty_bonus=0.0, max_prims=1, max_depth=-1, threads=0):
        h = C.c_void_p()
        if kd_aware:
            prm = None if isect_cost is None else C.byref(BspPaperKdParams(isect_cost, trav_cost, kd_trav_cost, empty_bonus, max_prims, max_depth, threads))
            _check(lib.hprt_bsppaperkdinst_build(model._h, prm, C.byref(h)))
        else:
            prm = None if isect_cost is None else C.byref(BspPaperParams(isect_cost, trav_cost, empty_bonus, max_prims, max_depth, threads))
            _check(lib.hprt_bsppaperinst_build(model._h, prm, C.byref(h)))
        self._h = h


class BspNodeParams(C.Structure):
    """HprtBspNodeParams: chooser and form (the accelerator's name), K, the seed, the parameters of the nine
    Create...TreeAccelerator functions and the builder's thread count."""
    _fields_ = [("chooser", C.c_int), ("form", C.c_int), ("n_directions", C.c_int), ("seed", C.c_uint32), ("isect_cost", C.c_int), ("trav_cost", C.c_int),
                ("kd_trav_cost", C.c_int), ("empty_bonus", C.c_float), ("max_prims", C.c_int), ("max_depth", C.c_int), ("threads", C.c_int)]


BSPNODE_CHOOSERS = ("arbitrary", "cluster", "random")      # HPRT_BSPNODE_ARBITRARY / _CLUSTER / _RANDOM
BSPNODE_FORMS = ("", "withkd", "fastkd")                   # HPRT_BSPNODE_PLAIN / _WITHKD / _FASTKD
BSPNODE_DEFAULT_SEED = 5489                                # HPRT_BSPNODE_DEFAULT_SEED: std::mt19937's own default
BSPNODE_ACCELERATORS = tuple("bsp" + c + f for c in BSPNODE_CHOOSERS for f in BSPNODE_FORMS)


def _bspnode_params(accelerator, fastkd, n_directions, seed, isect_cost, trav_cost, kd_trav_cost, empty_bonus, max_prims, max_depth, threads):
    """HprtBspNodeParams of an accelerator name ("bspcluster", "bsprandomwithkd", ...); fastkd: the form the builder takes"""
    if accelerator not in BSPNODE_ACCELERATORS:
        raise ValueError("%r is no node-based BSP accelerator (%s)" % (accelerator, ", ".join(BSPNODE_ACCELERATORS)))
    k = BSPNODE_ACCELERATORS.index(accelerator)
    if (k % 3 == 2) != fastkd:
        raise ValueError("%r is built by %s" % (accelerator, "BspNode" if fastkd else "BspNodeKd"))
    return BspNodeParams(k // 3, k % 3, n_directions, seed, isect_cost, trav_cost, kd_trav_cost, empty_bonus, max_prims, max_depth, threads)


class BspNode(BspPaper):
    """Node-based BSP tree, plain or withkd form (host): Create{BSPArbitrary,BSPCluster,BSPRandom}[WithKd]TreeAccelerator(prims,
    params) — the reference's BSP over BSPNode, so a BspPaper in all but its builder: info(), arrays() and Scene.attach_bsppaper
    take it unchanged.  BspNode(model) takes accelerator and parameters from the scene's Accelerator line; given `accelerator`
    ("bspcluster", "bsprandomwithkd", ...), the keyword parameters replace it.  `seed` seeds the direction chooser's std::mt19937
    (the reference seeds from std::random_device): the same seed gives the same tree.  device: None builds on the host; a HIP
    device ordinal costs the split candidates of nodes with at least min_candidates candidates on that GPU (k_sweepcost; the same
    tree, byte for byte) and leaves HprtBuildDeviceStats as a dict in self.build_stats.  max_edges / max_faces / max_face_edges: 0,
    or a value that lowers the kernel's compiled capacity."""

    def __init__(self, model=None, accelerator=None, handle=None, n_directions=3, seed=BSPNODE_DEFAULT_SEED, isect_cost=80, trav_cost=5,
                 empty_bonus=0.0, max_prims=1, max_depth=-1, threads=0, device=None, min_candidates=0, max_edges=0, max_faces=0, max_face_edges=0, build_stats=None):
        self.build_stats = build_stats
        if handle is None:
            prm = None if accelerator is None else C.byref(_bspnode_params(accelerator, False, n_directions, seed, isect_cost, trav_cost, 1, empty_bonus,
                                                                          max_prims, max_depth, threads))
            handle, self.build_stats = _build_tree("bspnode", "build", (model._h,), prm,
                                                   _device_opts(BspBuildDeviceOpts, device, min_candidates, max_edges, max_faces, max_face_edges, 0))
        self._h = handle

    @staticmethod
    def from_triangles(p9, accelerator, n_directions=3, seed=BSPNODE_DEFAULT_SEED, isect_cost=80, trav_cost=5, empty_bonus=0.0, max_prims=1,
                       max_depth=-1, threads=0, device=None, min_candidates=0, max_edges=0, max_faces=0, max_face_edges=0):
        """p9: [n, 9] (or [n, 3, 3]) float32 world-space triangle vertices in creation order.  device ...: as in the constructor."""
        p9 = np.ascontiguousarray(p9, np.float32).reshape(-1, 9)
        prm = _bspnode_params(accelerator, False, n_directions, seed, isect_cost, trav_cost, 1, empty_bonus, max_prims, max_depth, threads)
        h, st = _build_tree("bspnode", "build_from_triangles", (p9.shape[0], _ptr(p9)), C.byref(prm),
                            _device_opts(BspBuildDeviceOpts, device, min_candidates, max_edges, max_faces, max_face_edges, 0))
        return BspNode(handle=h, build_stats=st)


class BspNodeKd(BspPaperKd):
    """Node-based BSP tree, fastkd form (host): Create{BSPArbitrary,BSPCluster,BSPRandom}FastKdTreeAccelerator(prims, params) — the
    reference's BSPKd over BSPKdNode, so a BspPaperKd in all but its builder: Scene.attach_bsppaperkd takes it unchanged.
    Arguments as BspNode's (device, min_candidates and the capacities included), plus kd_trav_cost."""

    def __init__(self, model=None, accelerator=None, handle=None, n_directions=3, seed=BSPNODE_DEFAULT_SEED, isect_cost=80, trav_cost=5,
                 kd_trav_cost=1, empty_bonus=0.0, max_prims=1, max_depth=-1, threads=0, device=None, min_candidates=0, max_edges=0, max_faces=0, max_face_edges=0, build_stats=None):
        self.build_stats = build_stats
        if handle is None:
            prm = None if accelerator is None else C.byref(_bspnode_params(accelerator, True, n_directions, seed, isect_cost, trav_cost, kd_trav_cost,
                                                                          empty_bonus, max_prims, max_depth, threads))
            handle, self.build_stats = _build_tree("bspnodekd", "build", (model._h,), prm,
                                                   _device_opts(BspBuildDeviceOpts, device, min_candidates, max_edges, max_faces, max_face_edges, 0))
        self._h = handle

    @staticmethod
    def from_triangles(p9, accelerator, n_directions=3, seed=BSPNODE_DEFAULT_SEED, isect_cost=80, trav_cost=5, kd_trav_cost=1, empty_bonus=0.0,
                       max_prims=1, max_depth=-1, threads=0, device=None, min_candidates=0, max_edges=0, max_faces=0, max_face_edges=0):
        """p9: [n, 9] (or [n, 3, 3]) float32 world-space triangle vertices in creation order.  device ...: as in the constructor."""
        p9 = np.ascontiguousarray(p9, np.float32).reshape(-1, 9)
        prm = _bspnode_params(accelerator, True, n_directions, seed, isect_cost, trav_cost, kd_trav_cost, empty_bonus, max_prims, max_depth, threads)
        h, st = _build_tree("bspnodekd", "build_from_triangles", (p9.shape[0], _ptr(p9)), C.byref(prm),
                            _device_opts(BspBuildDeviceOpts, device, min_candidates, max_edges, max_faces, max_face_edges, 0))
        return BspNodeKd(handle=h, build_stats=st)


def bspnode_tree(model, accelerator=None, **kw):
    """The node-based BSP tree of `accelerator` (default: the scene's Accelerator line) and the Scene method that attaches it:
    (BspNodeKd, "attach_bsppaperkd") for the fastkd forms, (BspNode, "attach_bsppaper") for the others.  kw: the builders' keywords,
    device=, min_candidates=, max_edges=, max_faces= and max_face_edges= of the device-assisted build among them."""
    name = accelerator if accelerator is not None else model.accelerator
    fastkd = name.endswith("fastkd")
    if not fastkd:
        kw.pop("kd_trav_cost", None)
    return (BspNodeKd if fastkd else BspNode)(model, accelerator, **kw), ("attach_bsppaperkd" if fastkd else "attach_bsppaper")


class BspNodeInst(BspPaperInst):
    """Two-level node-based BSP trees (host) of a model WITH object instances, as pbrtObjectInstance and pbrtWorldEnd build them under
    one of the nine node-based accelerators (core/api.cpp:1794-1819): one tree per object of more than one primitive and the
    top-level tree over the top-level items, an instance a primitive with a zero normal and its world bound.  A BspPaperInst in all
    but its builder — kd-aware for the fastkd forms — so info(), copy(), object_copy(), set_tree() and Scene.attach_bsppaperinst take
    it unchanged.  BspNodeInst(model) takes accelerator and parameters from the scene's Accelerator line; given `accelerator`
    ("bspcluster", "bsprandomfastkd", ...), the keyword parameters replace it.  Every tree starts a fresh std::mt19937(seed).
    device: None builds on the host; a HIP device ordinal costs the split candidates of nodes with at least min_candidates candidates
    on that GPU (k_sweepcost, one session for all trees; the same trees, byte for byte) and leaves HprtBuildDeviceStats, summed over
    the trees, as a dict in self.build_stats.  max_edges / max_faces / max_face_edges: 0, or a value that lowers the kernel's
    compiled capacity."""

    def __init__(self, model, accelerator=None, n_directions=3, seed=BSPNODE_DEFAULT_SEED, isect_cost=80, trav_cost=5, kd_trav_cost=1,
                 empty_bonus=0.0, max_prims=1, max_depth=-1, threads=0, device=None, min_candidates=0, max_edges=0, max_faces=0, max_face_edges=0):
        prm = None
        if accelerator is not None:
            prm = C.byref(_bspnode_params(accelerator, accelerator.endswith("fastkd"), n_directions, seed, isect_cost, trav_cost, kd_trav_cost,
                                          empty_bonus, max_prims, max_depth, threads))
        self._h, self.build_stats = _build_tree("bspnodeinst", "build", (model._h,), prm,
                                                _device_opts(BspBuildDeviceOpts, device, min_candidates, max_edges, max_faces, max_face_edges, 0))


class Scene:
    """Device-resident scene: Aggregate (Intersect/IntersectP) + Integrator (Render)."""

    def __init__(self, model, bvh, device=-1):
        h = C.c_void_p()
        _check(lib.hprt_scene_create_from_model(model._h, bvh._h, device, C.byref(h)))
        self._h = h
        self._model = model

    @staticmethod
    def from_desc(desc, device=-1):
        """hprt_scene_create on a caller-filled SceneDesc (borrowed host pointers; the library copies everything to HBM) —
        the entry a BVHAccel-shaped adapter inside pbrt uses."""
        h = C.c_void_p()
        _check(lib.hprt_scene_create(C.byref(desc), device, C.byref(h)))
        sc = Scene.__new__(Scene)
        sc._h = h
        sc._model = None
        return sc

    def attach_kdtree(self, kdtree):
        """hprt_scene_attach_kdtree: every later trace and render walks `kdtree` (built over this scene's primitives)."""
        _check(lib.hprt_scene_attach_kdtree(self._h, kdtree._h))
        self._kdtree = kdtree

    def attach_kdinst(self, kdinst):
        """hprt_scene_attach_kdinst: every later trace and render of this INSTANCED scene walks the two-level kd-trees `kdinst`
        (a KdInst of the model the scene was made of).  Counters and pixel statistics follow the kd scene's, summed over both levels."""
        _check(lib.hprt_scene_attach_kdinst(self._h, kdinst._h))
        self._kdinst = kdinst

    def attach_rbspinst(self, rbspinst):
        """hprt_scene_attach_rbspinst: every later trace and render of this INSTANCED scene walks the two-level RBSP trees `rbspinst`
        (an RbspInst of the model the scene was made of).  Counters and pixel statistics follow the rbsp scene's — for kd-aware trees
        the rbspkd scene's, with kd_counters() and pixel_kd_stats() — summed over both levels."""
        _check(lib.hprt_scene_attach_rbspinst(self._h, rbspinst._h))
        self._rbspinst = rbspinst

    def attach_bsppaperinst(self, bsppaperinst):
        """hprt_scene_attach_bsppaperinst: every later trace and render of this INSTANCED scene walks the two-level general BSP trees
        `bsppaperinst` (a BspPaperInst of this scene's model); kd-aware trees count their kd share like a bsppaperkd scene."""
        _check(lib.hprt_scene_attach_bsppaperinst(self._h, bsppaperinst._h))
        self._bsppaperinst = bsppaperinst

    def attach_rbsp(self, rbsp):
        """hprt_scene_attach_rbsp: every later trace and render walks `rbsp` (built over this scene's primitives); replaces an
        attached kd-tree."""
        _check(lib.hprt_scene_attach_rbsp(self._h, rbsp._h))
        self._rbsp = rbsp

    def attach_rbspkd(self, rbspkd):
        """hprt_scene_attach_rbspkd: every later trace and render walks `rbspkd` (an RbspKd over this scene's primitives);
        replaces an attached kd-tree or RBSP tree."""
        _check(lib.hprt_scene_attach_rbspkd(self._h, rbspkd._h))
        self._rbspkd = rbspkd

    def attach_bsppaper(self, bsppaper):
        """hprt_scene_attach_bsppaper: every later trace and render walks `bsppaper` (a BspPaper over this scene's primitives);
        replaces any attached tree.  Pixel statistics are bspTreeNodeTraversals[P] (ACCEL_BSP)."""
        _check(lib.hprt_scene_attach_bsppaper(self._h, bsppaper._h))
        self._bsppaper = bsppaper

    def attach_bsppaperkd(self, bsppaperkd):
        """hprt_scene_attach_bsppaperkd: every later trace and render walks `bsppaperkd` (a BspPaperKd over this scene's
        primitives); replaces any attached tree.  Counters and pixel statistics follow the rbspkd scene's (kd_counters,
        pixel_kd_stats, write_pixel_stats_rbspkd)."""
        _check(lib.hprt_scene_attach_bsppaperkd(self._h, bsppaperkd._h))
        self._bsppaperkd = bsppaperkd

    def kd_counters(self):
        """(kdTreeNodeTraversals, kdTreeNodeTraversalsP) of the last counting trace or render of an rbspkd or bsppaperkd scene
        (zeros otherwise); the counters' [1] / nodes_entered[_p] hold kd and oblique interior nodes together."""
        out = np.zeros(2, np.uint64)
        _check(lib.hprt_scene_kd_counters(self._h, _ptr(out)))
        return int(out[0]), int(out[1])

    def intersect(self, o, d, tmax, count=False):
        o = np.ascontiguousarray(o, np.float32); d = np.ascontiguousarray(d, np.float32)
        tmax = np.ascontiguousarray(tmax, np.float32)
        n = tmax.shape[0]
        t = np.zeros(n, np.float32); prim = np.zeros(n, np.int32); bary = np.zeros((n, 3), np.float32)
        ctr = np.zeros(4, np.uint64) if count else None
        _check(lib.hprt_intersect(self._h, n, _ptr(o), _ptr(d), _ptr(tmax), _ptr(t), _ptr(prim), _ptr(bary), _ptr(ctr)))
        return (t, prim, bary, ctr) if count else (t, prim, bary)

    def intersect_instanced(self, o, d, tmax, count=False):
        """As intersect, plus the instance each hit went through (-1: none); prim numbers the ordered
        primitives of all aggregates (top level, then object 0, 1, ...)."""
        o = np.ascontiguousarray(o, np.float32); d = np.ascontiguousarray(d, np.float32)
        tmax = np.ascontiguousarray(tmax, np.float32)
        n = tmax.shape[0]
        t = np.zeros(n, np.float32); prim = np.zeros(n, np.int32); inst = np.zeros(n, np.int32); bary = np.zeros((n, 3), np.float32)
        ctr = np.zeros(4, np.uint64) if count else None
        _check(lib.hprt_intersect_instanced(self._h, n, _ptr(o), _ptr(d), _ptr(tmax), _ptr(t), _ptr(prim), _ptr(inst), _ptr(bary), _ptr(ctr)))
        return (t, prim, inst, bary, ctr) if count else (t, prim, inst, bary)

    def occluded(self, o, d, tmax, count=False):
        o = np.ascontiguousarray(o, np.float32); d = np.ascontiguousarray(d, np.float32)
        tmax = np.ascontiguousarray(tmax, np.float32)
        n = tmax.shape[0]
        occ = np.zeros(n, np.uint8)
        ctr = np.zeros(4, np.uint64) if count else None
        _check(lib.hprt_occluded(self._h, n, _ptr(o), _ptr(d), _ptr(tmax), _ptr(occ), _ptr(ctr)))
        return (occ, ctr) if count else occ

    def shadow_grid_info(self):
        """Test hook (not part of include/hprt.h): the scene's light-centred shadow grid — eligible (False: its shadow rays take the walk),
        R, entries, near (near-list length), bytes, build_seconds, longest and mean list, light (the point every ray must end at), render_launches
        (launches of k_shadow_grid by this scene's renders so far)."""
        out = np.zeros(12, np.float64)
        _check(lib.hprt_debug_shadow_grid_info(self._h, _ptr(out)))
        return {"eligible": bool(out[0]), "R": int(out[1]), "entries": int(out[2]), "near": int(out[3]), "bytes": int(out[4]), "build_seconds": float(out[5]),
                "longest": int(out[6]), "mean": float(out[7]), "light": out[8:11].astype(np.float32), "render_launches": int(out[11])}

    def _grid_image(self, read, info, faces):
        words = np.zeros(2, np.uint64)
        _check(read(self._h, _ptr(words), None, 0, None, 0))
        blocks = np.zeros(int(words[0]), np.uint32); records = np.zeros(max(1, int(words[1])), np.uint32)
        _check(read(self._h, _ptr(words), _ptr(blocks), blocks.size, _ptr(records), records.size))
        return shadow_grid_image_decode(blocks, records[:int(words[1])], info["R"], info["near"], faces=faces)

    def _grid_occluded(self, occluded, n, rays7_ptr, occ_ptr):
        ms = C.c_float()
        _check(occluded(self._h, n, rays7_ptr, occ_ptr, C.byref(ms)))
        return float(ms.value)

    def shadow_grid_image(self):
        """Test hook (not part of include/hprt.h): the image k_shadow_grid reads of this scene, copied back from the device and decoded as
        shadow_grid_image_decode does."""
        return self._grid_image(lib.hprt_debug_shadow_grid_image_read, self.shadow_grid_info(), 6)

    def shadow_grid_occluded_device(self, n, rays7_ptr, occ_ptr):
        """Test hook (not part of include/hprt.h): k_shadow_grid on n device rays ([7][n] planes) that all end at the scene's light,
        d = float32(light - o); returns the kernel's milliseconds."""
        return self._grid_occluded(lib.hprt_debug_shadow_grid_occluded, n, rays7_ptr, occ_ptr)

    def distant_grid_info(self):
        """Test hook (not part of include/hprt.h): the scene's light-aligned shadow grid of its one distant light — eligible (False: its
        shadow rays take the walk), R, entries, near, bytes, build_seconds, pack_seconds, longest and mean list, w (towards the light), U, V
        (the frame the cells lie in), render_launches (launches of k_distant_grid by this scene's renders so far), eps."""
        out = np.zeros(20, np.float64)
        _check(lib.hprt_debug_distant_grid_info(self._h, _ptr(out)))
        return {"eligible": bool(out[0]), "R": int(out[1]), "entries": int(out[2]), "near": int(out[3]), "bytes": int(out[4]), "build_seconds": float(out[5]),
                "pack_seconds": float(out[6]), "longest": int(out[7]), "mean": float(out[8]), "w": out[9:12].astype(np.float32), "U": out[12:15].astype(np.float32),
                "V": out[15:18].astype(np.float32), "render_launches": int(out[18]), "eps": float(out[19])}

    def distant_grid_image(self):
        """Test hook (not part of include/hprt.h): the image k_distant_grid reads of this scene, copied back from the device and decoded as
        shadow_grid_image_decode does (faces = 1)."""
        return self._grid_image(lib.hprt_debug_distant_grid_image_read, self.distant_grid_info(), 1)

    def distant_grid_occluded_device(self, n, rays7_ptr, occ_ptr):
        """Test hook (not part of include/hprt.h): k_distant_grid on n device rays ([7][n] planes) formed as a render forms the shadow
        rays of the scene's distant light; returns the kernel's milliseconds."""
        return self._grid_occluded(lib.hprt_debug_distant_grid_occluded, n, rays7_ptr, occ_ptr)

    def intersect_device(self, n, rays7_ptr, t_ptr, prim_ptr, bary_ptr=None, stream=None):
        _check(lib.hprt_intersect_device(self._h, n, rays7_ptr, t_ptr, prim_ptr, bary_ptr, stream))

    def occluded_device(self, n, rays7_ptr, occ_ptr, stream=None):
        _check(lib.hprt_occluded_device(self._h, n, rays7_ptr, occ_ptr, stream))

    def render(self, opt=None, tile_begin=0, tile_end=0, tile_stride=1, spp_chunk=0, count_work=False, film_ptr=None,
               stream=None, pixel_stats=False, count_traced=False, trace_all=False, export_foreign=False):
        """Render(): returns (film_xyzw [H,W,4] float32 or None when film_ptr is given, stats dict)."""
        opt = opt or self._model.options
        desc = RenderDesc()
        desc.opt = opt
        desc.tile_begin, desc.tile_end, desc.tile_stride = tile_begin, tile_end, tile_stride
        desc.spp_chunk = spp_chunk
        # count_traced / trace_all: see HPRT_RENDER_COUNT_TRACED / HPRT_RENDER_TRACE_ALL in include/hprt.h
        desc.flags = (RENDER_COUNT_WORK if count_work else 0) | (RENDER_PIXEL_STATS if pixel_stats else 0) | \
                     (RENDER_COUNT_TRACED if count_traced else 0) | (RENDER_TRACE_ALL if trace_all else 0) | \
                     (RENDER_EXPORT_FOREIGN if export_foreign else 0)      # export_foreign: see film_records() / Comm.film_gather()
        self._film_shape = tuple(int(v) for v in (opt.film_bounds()[3] - opt.film_bounds()[1], opt.film_bounds()[2] - opt.film_bounds()[0]))
        st = RenderStats()
        _check(lib.hprt_render(self._h, C.byref(desc), film_ptr, stream, C.byref(st)))
        film = None
        if film_ptr is None:
            x0, y0, x1, y1 = opt.film_bounds()
            film = np.zeros((y1 - y0, x1 - x0, 4), np.float32)
            _check(lib.hprt_film_read(self._h, _ptr(film), film.shape[0] * film.shape[1]))
        return film, st.as_dict()

    def render_ao(self, n_samples=64, cos_sample=True, opt=None, tile_begin=0, tile_end=0, tile_stride=1, spp_chunk=0, count_work=False,
                  film_ptr=None, stream=None):
        """hprt_render_ao: Render() with AOIntegrator::Li (integrators/ao.cpp) as the estimator; returns what render() returns."""
        opt = opt or self._model.options
        desc = RenderDesc()
        desc.opt = opt
        desc.tile_begin, desc.tile_end, desc.tile_stride = tile_begin, tile_end, tile_stride
        desc.spp_chunk = spp_chunk
        desc.flags = RENDER_COUNT_WORK if count_work else 0
        ao = AoParams(int(n_samples), int(bool(cos_sample)))
        st = RenderStats()
        _check(lib.hprt_render_ao(self._h, C.byref(desc), C.byref(ao), film_ptr, stream, C.byref(st)))
        self._film_shape = tuple(int(v) for v in (opt.film_bounds()[3] - opt.film_bounds()[1], opt.film_bounds()[2] - opt.film_bounds()[0]))
        film = None
        if film_ptr is None:
            x0, y0, x1, y1 = opt.film_bounds()
            film = np.zeros((y1 - y0, x1 - x0, 4), np.float32)
            _check(lib.hprt_film_read(self._h, _ptr(film), film.shape[0] * film.shape[1]))
        return film, st.as_dict()

    @staticmethod
    def _direct_args(strategy, max_depth, n_light_samples):
        dp = DirectParams({"all": 0, "one": 1}.get(strategy, strategy), int(max_depth))
        counts = None if n_light_samples is None else np.ascontiguousarray(n_light_samples, np.int32)
        return dp, counts

    def render_direct(self, strategy="all", max_depth=5, n_light_samples=None, n_lights=None, opt=None, tile_begin=0, tile_end=0, tile_stride=1, spp_chunk=0,
                      count_work=False, film_ptr=None, stream=None, flags=None):
        """hprt_render_direct: Render() with DirectLightingIntegrator::Li (integrators/directlighting.cpp) as the estimator; returns what
        render() returns.  n_light_samples: one count per scene light (Model.direct()), None: all 1 — n_lights then says how many lights
        the caller believes the scene has (default: the model's)."""
        opt = opt or self._model.options
        desc = RenderDesc()
        desc.opt = opt
        desc.tile_begin, desc.tile_end, desc.tile_stride = tile_begin, tile_end, tile_stride
        desc.spp_chunk = spp_chunk
        desc.flags = (RENDER_COUNT_WORK if count_work else 0) if flags is None else flags
        dp, counts = self._direct_args(strategy, max_depth, n_light_samples)
        if n_lights is None:
            n_lights = counts.shape[0] if counts is not None else self._model.counts()["lights"]
        st = RenderStats()
        _check(lib.hprt_render_direct(self._h, C.byref(desc), C.byref(dp), None if counts is None else _ptr(counts), int(n_lights), film_ptr, stream, C.byref(st)))
        self._film_shape = tuple(int(v) for v in (opt.film_bounds()[3] - opt.film_bounds()[1], opt.film_bounds()[2] - opt.film_bounds()[0]))
        film = None
        if film_ptr is None:
            x0, y0, x1, y1 = opt.film_bounds()
            film = np.zeros((y1 - y0, x1 - x0, 4), np.float32)
            _check(lib.hprt_film_read(self._h, _ptr(film), film.shape[0] * film.shape[1]))
        return film, st.as_dict()

    def dl_kernel_seconds(self):
        """Measurement hook (not part of include/hprt.h): HIP-event seconds of (k_dl_shade, k_dl_rays, k_dl_resolve, k_dl_advance) in the last
        render_direct, and the tree-walk steps its batches took."""
        out = np.zeros(5, np.float64)
        _check(lib.hprt_debug_dl_kernel_seconds(self._h, _ptr(out)))
        return tuple(float(v) for v in out[:4]), int(out[4])

    def sample_direct(self, px, py, sample, strategy="all", max_depth=5, n_light_samples=None, n_lights=None, opt=None):
        """hprt_sample_direct: L of individual camera samples under the direct-lighting estimator, [n, 3] float32."""
        opt = opt or self._model.options
        px = np.ascontiguousarray(px, np.int32); py = np.ascontiguousarray(py, np.int32)
        sample = np.ascontiguousarray(sample, np.int64)
        L = np.zeros((px.shape[0], 3), np.float32)
        dp, counts = self._direct_args(strategy, max_depth, n_light_samples)
        if n_lights is None:
            n_lights = counts.shape[0] if counts is not None else self._model.counts()["lights"]
        _check(lib.hprt_sample_direct(self._h, C.byref(opt), C.byref(dp), None if counts is None else _ptr(counts), int(n_lights), px.shape[0], _ptr(px), _ptr(py),
                                      _ptr(sample), _ptr(L)))
        return L

    def ao_kernel_seconds(self):
        """Measurement hook (not part of include/hprt.h): HIP-event seconds of (k_ao_frame, k_ao_rays, k_ao_resolve) in the last render_ao."""
        out = np.zeros(3, np.float64)
        _check(lib.hprt_debug_ao_kernel_seconds(self._h, _ptr(out)))
        return tuple(float(v) for v in out)

    def sample_ao(self, px, py, sample, n_samples, cos_sample, opt=None):
        """hprt_sample_ao: L of individual camera samples under the ambient-occlusion estimator, [n, 3] float32."""
        opt = opt or self._model.options
        px = np.ascontiguousarray(px, np.int32); py = np.ascontiguousarray(py, np.int32)
        sample = np.ascontiguousarray(sample, np.int64)
        L = np.zeros((px.shape[0], 3), np.float32)
        ao = AoParams(int(n_samples), int(bool(cos_sample)))
        _check(lib.hprt_sample_ao(self._h, C.byref(opt), C.byref(ao), px.shape[0], _ptr(px), _ptr(py), _ptr(sample), _ptr(L)))
        return L

    def reserve(self, opt=None, tile_begin=0, tile_end=0, tile_stride=1, spp_chunk=0):
        """hprt_scene_reserve: allocate the workspace of the coming render now (a host that renders once pays it at load)."""
        desc = RenderDesc()
        desc.opt = opt or self._model.options
        desc.tile_begin, desc.tile_end, desc.tile_stride, desc.spp_chunk, desc.flags = tile_begin, tile_end, tile_stride, spp_chunk, 0
        _check(lib.hprt_scene_reserve(self._h, C.byref(desc)))

    def debug_poison(self, byte):
        """Test hook (not part of include/hprt.h): fill every scratch stream, queue and stack with `byte` before each render
        (None switches it off).  A film that changes under it means a render consumed a word it never wrote."""
        lib.hprt_debug_poison_workspace.argtypes = [C.c_void_p, C.c_int]
        _check(lib.hprt_debug_poison_workspace(self._h, -1 if byte is None else int(byte)))

    def debug_device_halton(self, bounds_w, bounds_h, index, dim, sample_pixel_center=False, use_lds=False):
        """Test hook (not part of include/hprt.h): the device's halton_dim(index[i], dim[i]) of a sampler over bounds_w x bounds_h sample
        bounds, read from this scene's tables; use_lds: through the workgroup's LDS copy, as k_shade reads dimensions below 64."""
        index = np.ascontiguousarray(index, np.uint64); dim = np.ascontiguousarray(dim, np.int32)
        assert index.shape == dim.shape and index.ndim == 1
        out = np.zeros(index.shape[0], np.float32)
        _check(_probe().hprt_debug_device_halton(self._h, int(bounds_w), int(bounds_h), int(bool(sample_pixel_center)), int(bool(use_lds)),
                                                 index.shape[0], _ptr(index), _ptr(dim), _ptr(out)))
        return out

    def debug_device_bsdf(self, mode, shape, frame9, wo, wi, u):
        """Test hook (not part of include/hprt.h): the device BSDF of shapes[shape[i]]'s material at the frame frame9[i] (n, shading.n,
        shading.dpdu), no texture overrides.  mode 0: (material type, bsdf_num, eta); 1: bsdf_f; 2: bsdf_pdf; 3 / 4: bsdf_sample with
        all = false / true: f, wi, pdf, sampledType, the last three preset to (9, 9, 9), -7 and -1.  Returns float32 [n, 8]."""
        shape = np.ascontiguousarray(shape, np.int32)
        frame9 = np.ascontiguousarray(frame9, np.float32).reshape(-1, 9)
        wo = np.ascontiguousarray(wo, np.float32).reshape(-1, 3); wi = np.ascontiguousarray(wi, np.float32).reshape(-1, 3)
        u = np.ascontiguousarray(u, np.float32).reshape(-1, 2)
        n = shape.shape[0]
        assert shape.ndim == 1 and frame9.shape[0] == n and wo.shape[0] == n and wi.shape[0] == n and u.shape[0] == n
        out = np.zeros((n, 8), np.float32)
        _check(_probe().hprt_debug_device_bsdf(self._h, int(mode), n, _ptr(shape), _ptr(frame9), _ptr(wo), _ptr(wi), _ptr(u), _ptr(out)))
        return out

    def debug_device_bsdf_specular(self, mask, shape, frame9, wo, u):
        """Test hook (not part of include/hprt.h): bsdf_sample_specular — BSDF::Sample_f under mask 17 (BSDF_REFLECTION | BSDF_SPECULAR) or 18
        (BSDF_TRANSMISSION | BSDF_SPECULAR) — of shapes[shape[i]]'s material at the frame frame9[i].  Returns float32 [n, 8]: f, wi, pdf (wi
        and pdf preset to (9, 9, 9) and -7), and 1 where the material can offer either mask a lobe."""
        shape = np.ascontiguousarray(shape, np.int32)
        frame9 = np.ascontiguousarray(frame9, np.float32).reshape(-1, 9)
        wo = np.ascontiguousarray(wo, np.float32).reshape(-1, 3)
        u = np.ascontiguousarray(u, np.float32).reshape(-1, 2)
        n = shape.shape[0]
        assert shape.ndim == 1 and frame9.shape[0] == n and wo.shape[0] == n and u.shape[0] == n
        out = np.zeros((n, 8), np.float32)
        _check(_probe().hprt_debug_device_bsdf_specular(self._h, int(mask), n, _ptr(shape), _ptr(frame9), _ptr(wo), _ptr(u), _ptr(out)))
        return out

    def film_records(self):
        """Cross-tile film contributions of the last render(export_foreign=True): FILM_RECORD array (HprtFilmRecord)."""
        n = C.c_size_t()
        _check(lib.hprt_film_records_read(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, FILM_RECORD)
        if n.value:
            _check(lib.hprt_film_records_read(self._h, _ptr(out), n.value, C.byref(n)))
        return out

    def pixel_stats(self):
        """[H, W, 7] uint64 Pixel::stats of the last render(pixel_stats=True): rays, primitiveIntersections[P],
        leafNodeTraversals[P], bvhTreeNodeTraversals[P] (the fork's heat-map data, core/film.cpp:170-264)."""
        h, w = self._film_shape
        out = np.zeros((h, w, 7), np.uint64)
        _check(lib.hprt_pixel_stats_read(self._h, _ptr(out), h * w))
        return out

    def pixel_kd_stats(self):
        """[2, H, W] uint64: the kd share (kdTreeNodeTraversals, kdTreeNodeTraversalsP) of pixel_stats()' slots 5 / 6 after
        render(pixel_stats=True) of an rbspkd or bsppaperkd scene."""
        h, w = self._film_shape
        out = np.zeros((2, h, w), np.uint64)
        _check(lib.hprt_pixel_kd_stats_read(self._h, _ptr(out), h * w))
        return out

    def sample_radiance(self, px, py, sample, opt=None):
        opt = opt or self._model.options
        px = np.ascontiguousarray(px, np.int32); py = np.ascontiguousarray(py, np.int32)
        sample = np.ascontiguousarray(sample, np.int64)
        L = np.zeros((px.shape[0], 3), np.float32)
        _check(lib.hprt_sample_radiance(self._h, C.byref(opt), px.shape[0], _ptr(px), _ptr(py), _ptr(sample), _ptr(L)))
        return L

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:      # (module globals are cleared at interpreter exit)
            lib.hprt_scene_destroy(self._h)
            self._h = None


class Comm:
    """RCCL communicator for the film gather (hprt_comm_*): one process per GPU.  Rank 0 draws `Comm.unique_id()`, the
    host program distributes the 128 bytes (bench.py: through torch.distributed's store), every rank constructs."""

    @staticmethod
    def unique_id():
        buf = (C.c_uint8 * COMM_ID_BYTES)()
        _check(lib.hprt_comm_unique_id(buf))
        return bytes(buf)

    def __init__(self, unique_id, rank, n_ranks, device=-1):
        if len(unique_id) != COMM_ID_BYTES:
            raise ValueError("unique id must be %d bytes" % COMM_ID_BYTES)
        h = C.c_void_p()
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(unique_id)
        _check(lib.hprt_comm_create(buf, rank, n_ranks, device, C.byref(h)))
        self._h = h

    def info(self):
        r, n, d = C.c_int(), C.c_int(), C.c_int()
        _check(lib.hprt_comm_info(self._h, C.byref(r), C.byref(n), C.byref(d)))
        return {"rank": r.value, "n_ranks": n.value, "device": d.value}

    def film_gather(self, scene, film_ptr, n_pixels, root=0, stream=None):
        """Film::MergeFilmTile across ranks (hprt_film_gather): ncclReduce of the films + ordered merge of the
        cross-tile records on the root.  Every rank's last render must have used export_foreign=True."""
        _check(lib.hprt_film_gather(self._h, scene._h, film_ptr, n_pixels, root, stream))

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:
            lib.hprt_comm_destroy(self._h)
            self._h = None


def film_gather_local(scenes, film_ptrs, n_pixels, root=0):
    """hprt_film_gather_local: one process, one Scene per GPU."""
    n = len(scenes)
    hs = (C.c_void_p * n)(*[s._h for s in scenes])
    fs = (C.c_void_p * n)(*[C.c_void_p(p) if p else None for p in (film_ptrs or [None] * n)])
    _check(lib.hprt_film_gather_local(hs, fs, n, n_pixels, root))


def film_records_merge(film_xyzw, records):
    """Adds cross-tile records (any ranks', any order) into a host film [H,W,4] in place, per pixel in source-tile order."""
    assert film_xyzw.dtype == np.float32 and film_xyzw.flags.c_contiguous
    rec = np.ascontiguousarray(records, FILM_RECORD).copy()
    _check(lib.hprt_film_records_merge(_ptr(film_xyzw), film_xyzw.size // 4, _ptr(rec), rec.shape[0]))
    return film_xyzw


def film_resolve(film_xyzw, scale=1.0):
    """Film::WriteImage arithmetic (core/film.cpp:266-303): [H,W,4] xyz+weight -> [H,W,3] linear RGB."""
    f = np.ascontiguousarray(film_xyzw, np.float32)
    rgb = np.zeros(f.shape[:-1] + (3,), np.float32)
    _check(lib.hprt_film_resolve(_ptr(f), f.size // 4, C.c_float(scale), _ptr(rgb)))
    return rgb


def write_pixel_stats(prefix, stats7):
    """Film::WriteGeneralStats: the fork's per-pixel text matrices, '<prefix>-<counter>.txt'."""
    stats7 = np.ascontiguousarray(stats7, np.uint64)
    _check(lib.hprt_write_pixel_stats(prefix.encode(), _ptr(stats7), stats7.shape[1], stats7.shape[0]))


def write_pixel_stats_accel(prefix, stats7, accel):
    """The same for a render of any accelerator (ACCEL_BVH; ACCEL_KDTREE: slots 5 / 6 are kdTreeNodeTraversals[P];
    ACCEL_RBSP / ACCEL_BSP: slots 5 / 6 are bspTreeNodeTraversals[P])."""
    stats7 = np.ascontiguousarray(stats7, np.uint64)
    _check(lib.hprt_write_pixel_stats_accel(prefix.encode(), _ptr(stats7), stats7.shape[1], stats7.shape[0], accel))


def write_pixel_stats_rbspkd(prefix, stats7, kd2):
    """The same for an rbspkd or bsppaperkd render: kdTreeNodeTraversals[P] from kd2 (Scene.pixel_kd_stats), bspTreeNodeTraversals[P] =
    slot 5 / 6 minus that share."""
    stats7 = np.ascontiguousarray(stats7, np.uint64)
    kd2 = np.ascontiguousarray(kd2, np.uint64)
    if kd2.shape != (2,) + stats7.shape[:2]:
        raise ValueError("kd2 must be [2, H, W] for stats7 of [H, W, 7]")
    _check(lib.hprt_write_pixel_stats_rbspkd(prefix.encode(), _ptr(stats7), _ptr(kd2), stats7.shape[1], stats7.shape[0]))


def write_pfm(path, rgb):
    a = np.ascontiguousarray(rgb, np.float32)
    _check(lib.hprt_write_pfm(path.encode(), _ptr(a), a.shape[1], a.shape[0]))


def halton_permutations():
    n = C.c_size_t()
    _check(lib.hprt_halton_permutations(None, 0, C.byref(n)))
    out = np.zeros(n.value, np.uint16)
    _check(lib.hprt_halton_permutations(_ptr(out), n.value, C.byref(n)))
    return out
