"""ctypes wrapper around tests/ao_reference.cpp, the test-side restatement of the reference's ambient-occlusion render
(AOIntegrator::Li, the sampler's array samples and the tile loop) over the oracle's headers.  Compiled with g++ into a per-process
temporary directory on first use — test infrastructure only."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTER_NAMES = ("nodes_fetched", "nodes_fetched_p", "nodes_entered", "nodes_entered_p", "tri_tests", "tri_tests_p",
                 "tri_hits", "tri_hits_p", "sphere_tests", "sphere_tests_p", "rays", "shadow_rays", "camera_rays")
_lib = None


def _load():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="aoref"), "libaoref.so")
        cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function",
               "-I", os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests", "ao_reference.cpp"), "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("ao_reference.cpp failed to build:\n" + r.stderr)
        L = C.CDLL(out)
        vp, i32, i64, sz = C.c_void_p, C.c_int, C.c_int64, C.c_size_t
        L.aoref_last_error.restype = C.c_char_p
        L.aoref_scene_load.restype = vp
        L.aoref_scene_load.argtypes = [C.c_char_p]
        L.aoref_scene_free.argtypes = [vp]
        L.aoref_set_film.argtypes = [vp, i32, i32, vp, i32, i32]
        L.aoref_bounds.argtypes = [vp, vp]
        L.aoref_render.argtypes = [vp, i32, i32, i32, i32, vp, vp]
        L.aoref_sample.argtypes = [vp, i32, i32, sz, vp, vp, vp, vp]
        L.aoref_rays.restype = i32
        L.aoref_rays.argtypes = [vp, i32, i32, i32, i32, i64, vp, vp, vp, vp, vp, vp]
        L.aoref_pixel_samples.argtypes = [vp, i32, i32, i32, vp, vp]
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class AoScene:
    """A baked scene under the restated ambient-occlusion integrator."""

    def __init__(self, baked_path):
        L = _load()
        h = L.aoref_scene_load(baked_path.encode())
        if not h:
            raise RuntimeError("ao_reference: " + L.aoref_last_error().decode())
        self._h = C.c_void_p(h)

    def set_film(self, xres=0, yres=0, crop=None, spp=0, sample_pixel_center=None):
        c = None if crop is None else np.ascontiguousarray(crop, np.float32)
        _load().aoref_set_film(self._h, xres, yres, _p(c), spp, -1 if sample_pixel_center is None else int(bool(sample_pixel_center)))

    def set_options(self, opt):
        """the film and sampler of an hprt RenderOptions"""
        self.set_film(int(opt.xres), int(opt.yres), [opt.crop[i] for i in range(4)], int(opt.spp), bool(opt.sample_pixel_center))

    def bounds(self):
        """(cropped pixel bounds x0 y0 x1 y1, sample bounds x0 y0 x1 y1)"""
        b = np.zeros(8, np.int32)
        _load().aoref_bounds(self._h, _p(b))
        return [int(v) for v in b[:4]], [int(v) for v in b[4:]]

    def render(self, n_samples, cos_sample, tile_begin=0, tile_stride=1):
        """(film_xyzw [H, W, 4] float32, counters dict)"""
        (x0, y0, x1, y1), _ = self.bounds()
        film = np.zeros((y1 - y0, x1 - x0, 4), np.float32)
        ctr = np.zeros(13, np.uint64)
        _load().aoref_render(self._h, int(n_samples), int(bool(cos_sample)), int(tile_begin), int(tile_stride), _p(film), _p(ctr))
        return film, dict(zip(COUNTER_NAMES, [int(v) for v in ctr]))

    def sample(self, px, py, sample, n_samples, cos_sample):
        px = np.ascontiguousarray(px, np.int32); py = np.ascontiguousarray(py, np.int32); sample = np.ascontiguousarray(sample, np.int64)
        L = np.zeros((px.shape[0], 3), np.float32)
        _load().aoref_sample(self._h, int(n_samples), int(bool(cos_sample)), px.shape[0], _p(px), _p(py), _p(sample), _p(L))
        return L

    def rays(self, px, py, sample, n_samples, cos_sample):
        """the hemisphere rays of one camera sample: (origins [k, 3], directions [k, 3], terms [k], Halton indices [n], u [n, 2]); k = 0 when
        the camera ray escaped, else n_samples"""
        n = int(n_samples)
        o = np.zeros((n, 3), np.float32); d = np.zeros((n, 3), np.float32); term = np.zeros(n, np.float32)
        index = np.zeros(n, np.uint64); u = np.zeros((n, 2), np.float32)
        flipped = C.c_int(0)
        k = _load().aoref_rays(self._h, n, int(bool(cos_sample)), int(px), int(py), int(sample), _p(o), _p(d), _p(term), _p(index), _p(u), C.byref(flipped))
        self.last_flipped = bool(flipped.value)      # Faceforward(isect.n, -ray.d) differed from isect.n at this sample's hit
        return o[:k], d[:k], term[:k], index, u

    def pixel_samples(self, px, py, n_samples, spp):
        """what the tile loop's sampler holds after StartPixel: (array samples [spp * n_samples, 2], camera-sample dimensions [spp, 5])"""
        u = np.zeros((int(spp) * int(n_samples), 2), np.float32); cam = np.zeros((int(spp), 5), np.float32)
        _load().aoref_pixel_samples(self._h, int(n_samples), int(px), int(py), _p(u), _p(cam))
        return u, cam

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.aoref_scene_free(self._h)
            self._h = None
