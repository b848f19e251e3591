"""ctypes wrapper around tests/dl_reference.cpp, the test-side restatement of the reference's direct-lighting render
(DirectLightingIntegrator::Li, UniformSampleAllLights / UniformSampleOneLight, SpecularReflect / SpecularTransmit, the sampler's
arrays and the tile loop) over the oracle's headers.  Compiled with g++ into a per-process temporary directory on first use — test
infrastructure only."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTER_NAMES = ("nodes_fetched", "nodes_fetched_p", "nodes_entered", "nodes_entered_p", "tri_tests", "tri_tests_p",
                 "tri_hits", "tri_hits_p", "sphere_tests", "sphere_tests_p", "rays", "shadow_rays", "camera_rays")
STRATEGY = {"all": 0, "one": 1}
MASK_REFLECT, MASK_TRANSMIT = 1 | 16, 2 | 16      # BSDF_REFLECTION | BSDF_SPECULAR, BSDF_TRANSMISSION | BSDF_SPECULAR
_lib = None


def _load():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="dlref"), "libdlref.so")
        cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function",
               "-I", os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests", "dl_reference.cpp"), "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("dl_reference.cpp failed to build:\n" + r.stderr)
        L = C.CDLL(out)
        vp, i32, sz = C.c_void_p, C.c_int, C.c_size_t
        L.dlref_last_error.restype = C.c_char_p
        L.dlref_scene_load.restype = vp
        L.dlref_scene_load.argtypes = [C.c_char_p]
        L.dlref_scene_free.argtypes = [vp]
        L.dlref_n_lights.argtypes = [vp]
        L.dlref_set_film.argtypes = [vp, i32, i32, vp, i32, i32]
        L.dlref_bounds.argtypes = [vp, vp]
        L.dlref_render.argtypes = [vp, i32, i32, vp, i32, i32, i32, vp, vp, vp, vp]
        L.dlref_sample.argtypes = [vp, i32, i32, vp, i32, sz, vp, vp, vp, vp]
        L.dlref_pixel_samples.argtypes = [vp, i32, i32, vp, i32, i32, i32, vp, vp, vp, vp]
        L.dlref_bsdf_specular.argtypes = [vp, i32, sz, vp, vp, vp, vp, vp]
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class DlScene:
    """A baked scene under the restated direct-lighting integrator."""

    def __init__(self, baked_path):
        L = _load()
        h = L.dlref_scene_load(baked_path.encode())
        if not h:
            raise RuntimeError("dl_reference: " + L.dlref_last_error().decode())
        self._h = C.c_void_p(h)
        self.n_lights = int(L.dlref_n_lights(self._h))
        self._spp = None

    def set_film(self, xres=0, yres=0, crop=None, spp=0, sample_pixel_center=None):
        c = None if crop is None else np.ascontiguousarray(crop, np.float32)
        _load().dlref_set_film(self._h, xres, yres, _p(c), spp, -1 if sample_pixel_center is None else int(bool(sample_pixel_center)))
        if spp > 0:
            self._spp = spp

    def set_options(self, opt):
        """the film and sampler of an hprt RenderOptions"""
        self.set_film(int(opt.xres), int(opt.yres), [opt.crop[i] for i in range(4)], int(opt.spp), bool(opt.sample_pixel_center))

    def bounds(self):
        """(cropped pixel bounds x0 y0 x1 y1, sample bounds x0 y0 x1 y1)"""
        b = np.zeros(8, np.int32)
        _load().dlref_bounds(self._h, _p(b))
        return [int(v) for v in b[:4]], [int(v) for v in b[4:]]

    def _counts(self, n_light_samples):
        c = np.ones(self.n_lights, np.int32) if n_light_samples is None else np.ascontiguousarray(n_light_samples, np.int32)
        return c, int(c.shape[0])

    def _ok(self, rc):
        if rc < 0:
            raise RuntimeError("dl_reference: " + _load().dlref_last_error().decode())
        return rc

    def render(self, strategy, max_depth, n_light_samples=None, tile_begin=0, tile_stride=1, spp=None):
        """(film_xyzw [H, W, 4] float32, counters dict — with "nodes_deep", "fallback_nodes", "samples_deep2" —, L [spp, sample-bounds H, W, 3]);
        spp: the film's samples per pixel (for the shape of L; what set_film / set_options set last)"""
        (x0, y0, x1, y1), (sx0, sy0, sx1, sy1) = self.bounds()
        spp = spp or self._spp
        film = np.zeros((y1 - y0, x1 - x0, 4), np.float32)
        ctr = np.zeros(13, np.uint64); cov = np.zeros(3, np.uint64)
        L3 = np.zeros((spp, sy1 - sy0, sx1 - sx0, 3), np.float32) if spp else None
        c, n = self._counts(n_light_samples)
        self._ok(_load().dlref_render(self._h, STRATEGY[strategy], int(max_depth), _p(c), n, int(tile_begin), int(tile_stride), _p(film), _p(ctr), _p(L3), _p(cov)))
        d = dict(zip(COUNTER_NAMES, [int(v) for v in ctr]))
        d.update(nodes_deep=int(cov[0]), fallback_nodes=int(cov[1]), samples_deep2=int(cov[2]))
        return film, d, L3

    def sample(self, px, py, sample, strategy, max_depth, n_light_samples=None):
        px = np.ascontiguousarray(px, np.int32); py = np.ascontiguousarray(py, np.int32); sample = np.ascontiguousarray(sample, np.int64)
        L = np.zeros((px.shape[0], 3), np.float32)
        c, n = self._counts(n_light_samples)
        self._ok(_load().dlref_sample(self._h, STRATEGY[strategy], int(max_depth), _p(c), n, px.shape[0], _p(px), _p(py), _p(sample), _p(L)))
        return L

    def pixel_samples(self, px, py, strategy, max_depth, n_light_samples, spp):
        """what the tile loop's sampler holds after Preprocess and StartPixel: (list of arrays [spp * size, 2], camera-sample dimensions and
        the Get2D behind them [spp, 7], the dimension that Get2D read from [spp])"""
        c, n = self._counts(n_light_samples)
        total = 2 * int(max_depth) * int(c.sum()) * int(spp) if strategy == "all" else 0
        u = np.zeros((max(1, total), 2), np.float32); sizes = np.zeros(max(1, 2 * int(max_depth) * n), np.int32)
        cam = np.zeros((int(spp), 7), np.float32); dim = np.zeros(int(spp), np.int32)
        k = self._ok(_load().dlref_pixel_samples(self._h, STRATEGY[strategy], int(max_depth), _p(c), n, int(px), int(py), _p(u), _p(sizes), _p(cam), _p(dim)))
        arrays, o = [], 0
        for a in range(k):
            m = int(sizes[a]) * int(spp)
            arrays.append(u[o:o + m].copy()); o += m
        return arrays, cam, dim

    def bsdf_specular(self, mask, shape, frame9, wo, u):
        shape = np.ascontiguousarray(shape, np.int32); frame9 = np.ascontiguousarray(frame9, np.float32).reshape(-1, 9)
        wo = np.ascontiguousarray(wo, np.float32).reshape(-1, 3); u = np.ascontiguousarray(u, np.float32).reshape(-1, 2)
        out = np.zeros((shape.shape[0], 8), np.float32)
        self._ok(_load().dlref_bsdf_specular(self._h, int(mask), shape.shape[0], _p(shape), _p(frame9), _p(wo), _p(u), _p(out)))
        return out

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.dlref_scene_free(self._h)
            self._h = None
