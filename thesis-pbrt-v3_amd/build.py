"""Builds thesis-pbrt-v3_amd/lib/libhprt.so: host C++ (g++) + HIP kernels (hipcc, gfx950).

Flags that matter for parity: -ffp-contract=off and no fast-math on BOTH compilers, so
every float operation is a single IEEE rounding in source order (Numerics).
"""
import concurrent.futures
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(HERE, "build")
LIB = os.path.join(HERE, "lib")
HOST_SRCS = ["pbrt_frontend.cpp", "loop_subdiv.cpp", "scene_io.cpp", "texture_io.cpp", "bvh_builder.cpp", "kdtree_builder.cpp", "rbsp_builder.cpp", "bsppaper_builder.cpp", "bspnode_builder.cpp", "bvhold_builder.cpp", "wide_bvh.cpp", "shadow_grid.cpp", "distant_grid.cpp", "halton_tables.cpp", "capi_host.cpp"]
# host code built by hipcc without an offload target (no code object): the float operations of the scene layout keep the code
# generator they had when they sat in capi_device.hip
HIPCC_HOST_SRCS = ["scene_layout.cpp"]
HIP_SRCS = ["device/kernels.hip", "device/kd_walk.hip", "device/rbsp_walk.hip", "device/rbspkd_walk.hip", "device/bsppaper_walk.hip", "device/bsppaperkd_walk.hip", "device/kdinst_walk.hip", "device/kdop_cost.hip", "device/rbspinst_walk.hip", "device/bsppaperinst_walk.hip", "device/bsp_cost.hip", "device/bspnode_cost.hip", "device/hlbvh_build.hip", "device/shadow_grid.hip", "capi_device.hip", "capi_gather.hip"]
# hipcc names every HIP translation unit by a CUID (the __hip_cuid_* symbol in its code object) that it otherwise hashes from
# the source's and the object's ABSOLUTE paths, so the code objects — and the sha256 profiles/rNN_counters.json is stamped
# with — would depend on where the tree is checked out.  Pinned to the values the stamped build derived: the same code
# objects, byte for byte, from any directory.
# (device/kd_walk.hip, device/rbsp_walk.hip, device/rbspkd_walk.hip, device/bsppaper_walk.hip, device/bsppaperkd_walk.hip, device/kdinst_walk.hip, device/kdop_cost.hip, device/rbspinst_walk.hip, device/bsppaperinst_walk.hip, device/bsp_cost.hip, device/bspnode_cost.hip, device/hlbvh_build.hip, device/shadow_grid.hip: values of their own, so that adding them left the other code
# objects as they were)
CUIDS = {"device/kernels.hip": "a6cd736c50efffab", "device/kd_walk.hip": "5c0d2e7f41b3a916", "device/rbsp_walk.hip": "3e91a5c07d2b84f6",
         "device/rbspkd_walk.hip": "7a4f0c2e9b61d385", "device/bsppaper_walk.hip": "c52e8b1d06f3a794",
         "device/bsppaperkd_walk.hip": "e8136d4a9f07c2b5", "device/kdinst_walk.hip": "4d9b27f1a60c8e53", "device/kdop_cost.hip": "b7e20a5c93d1f468",
         "device/rbspinst_walk.hip": "9f3c61d8b2047ae5", "device/bsppaperinst_walk.hip": "2c7e5a90d4b18f63", "device/bsp_cost.hip": "6b1f94c3e7a0d258",
         "device/bspnode_cost.hip": "d3a7150c8e4f92b6", "device/hlbvh_build.hip": "58e2c9a4f1b7063d", "device/shadow_grid.hip": "a17c3e58d90b24f6",
         "capi_device.hip": "1b24418c11488d5c", "capi_gather.hip": "89501e8167866ce2"}
# lib/libhprt_probe.so: device probes for the tests (device/halton_probe.hip: halton_dim over host arrays; device/bsdf_probe.hip: the
# BSDF functions over host arrays of queries), linked against libhprt.so.
# A library of its own, so that libhprt.so's .hip_fatbin — what profiles/rNN_counters.json is stamped with — gains no code object.
PROBE_SRCS = ["device/halton_probe.hip", "device/bsdf_probe.hip", "device/bsdf_specular_probe.hip"]
CUIDS["device/halton_probe.hip"] = "f04b8d61c2a79e35"
CUIDS["device/bsdf_probe.hip"] = "3d8a6f0b92e4c517"
CUIDS["device/bsdf_specular_probe.hip"] = "81c6f2d05a9e347b"
# lib/libhprt_ao.so: the ambient-occlusion kernels (device/ao.hip: k_ao_frame, k_ao_rays, k_ao_resolve and their launchers), which
# libhprt.so links against and finds beside itself ($ORIGIN).  A library of its own for the probes' reason: libhprt.so's .hip_fatbin
# gains no code object, so the stamp of the counter summaries still names the kernels they were measured on.
AO_SRCS = ["device/ao.hip"]
CUIDS["device/ao.hip"] = "c94e1a7b35f0d826"
# lib/libhprt_dl.so: the direct-lighting kernels (device/direct.hip: k_dl_shade, k_dl_rays, k_dl_resolve, k_dl_advance and their
# launchers), beside libhprt.so exactly as libhprt_ao.so is, and for its reason.
DL_SRCS = ["device/direct.hip"]
CUIDS["device/direct.hip"] = "5e0b93a7c42d16f8"
# lib/libhprt_dg.so: the distant light's shadow-grid kernel (device/distant_grid.hip: k_distant_grid and its launcher), beside
# libhprt.so exactly as libhprt_ao.so is, and for its reason.
DG_SRCS = ["device/distant_grid.hip"]
CUIDS["device/distant_grid.hip"] = "7d2f8b4e61a9c035"
COMMON = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function"]


def _hipcc():
    for c in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found")


def _newer(src_files, out):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(f) > t for f in src_files)


def _headers():
    hs = []
    for root, _, files in os.walk(CSRC):
        hs += [os.path.join(root, f) for f in files if f.endswith(".h")]
    hs.append(os.path.join(HERE, "..", "include", "hprt.h"))
    return hs


def build(verbose=False, force=False):
    os.makedirs(OBJ, exist_ok=True)
    os.makedirs(LIB, exist_ok=True)
    hipcc = _hipcc()
    headers = _headers()
    jobs = []
    for s in HOST_SRCS + HIPCC_HOST_SRCS:
        src = os.path.join(CSRC, s)
        obj = os.path.join(OBJ, s.replace("/", "_") + ".o")
        cmd = [hipcc if s in HIPCC_HOST_SRCS else "g++"] + COMMON + ["-c", src, "-o", obj]
        jobs.append((src, obj, cmd))
    for s in HIP_SRCS + AO_SRCS + DL_SRCS + DG_SRCS + PROBE_SRCS:
        src = os.path.join(CSRC, s)
        obj = os.path.join(OBJ, s.replace("/", "_") + ".o")
        cmd = [hipcc, "--offload-arch=gfx950"] + COMMON + ["-Wno-unused-result", "-cuid=" + CUIDS[s], "-c", src, "-o", obj]
        jobs.append((src, obj, cmd))

    def run(job):
        src, obj, cmd = job
        if not force and not _newer([src, os.path.abspath(__file__)] + headers, obj):   # (build.py: a changed flag rebuilds too)
            return None
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("compile failed: %s\n%s\n%s" % (" ".join(cmd), r.stdout, r.stderr))
        return r.stderr

    with concurrent.futures.ThreadPoolExecutor(max_workers=4) as ex:
        for out in ex.map(run, jobs):
            if verbose and out:
                print(out)
    lib = os.path.join(LIB, "libhprt.so")
    n_side = len(PROBE_SRCS) + len(DG_SRCS) + len(DL_SRCS) + len(AO_SRCS)
    probe_objs = [j[1] for j in jobs[len(jobs) - len(PROBE_SRCS):]]
    dg_objs = [j[1] for j in jobs[len(jobs) - len(PROBE_SRCS) - len(DG_SRCS):len(jobs) - len(PROBE_SRCS)]]
    dl_objs = [j[1] for j in jobs[len(jobs) - n_side + len(AO_SRCS):len(jobs) - n_side + len(AO_SRCS) + len(DL_SRCS)]]
    ao_objs = [j[1] for j in jobs[len(jobs) - n_side:len(jobs) - n_side + len(AO_SRCS)]]
    objs = [j[1] for j in jobs[:len(jobs) - n_side]]
    ao = os.path.join(LIB, "libhprt_ao.so")
    dl = os.path.join(LIB, "libhprt_dl.so")
    dg = os.path.join(LIB, "libhprt_dg.so")
    for side, side_objs in ((ao, ao_objs), (dl, dl_objs), (dg, dg_objs)):
        if force or _newer(side_objs, side):
            cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-o", side] + side_objs
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError("link failed: %s\n%s" % (" ".join(cmd), r.stderr))
    if force or _newer(objs + [ao, dl, dg], lib):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-o", lib] + objs + ["-L" + LIB, "-lhprt_ao", "-lhprt_dl", "-lhprt_dg", "-Wl,-rpath,$ORIGIN", "-lz", "-L/opt/rocm/lib", "-lrccl"]   # zlib: PNG textures (texture_io.cpp); RCCL: film gather (capi_gather.hip)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("link failed: %s\n%s" % (" ".join(cmd), r.stderr))
    probe = os.path.join(LIB, "libhprt_probe.so")
    if force or _newer(probe_objs + [lib], probe):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-o", probe] + probe_objs + ["-L" + LIB, "-lhprt", "-Wl,-rpath,$ORIGIN"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("link failed: %s\n%s" % (" ".join(cmd), r.stderr))
    return lib


if __name__ == "__main__":
    print(build(verbose="-v" in sys.argv, force="-f" in sys.argv))
