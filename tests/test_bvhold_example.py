"""examples/hprt_render.cpp on an Accelerator "bvhold" scene: the host program builds the tree with hprt_bvhold_build where it
builds the fork's BVH otherwise, and on a tie-free scene (tests/test_bvhold_host.py) its image is the "bvh" render's bit for bit."""
import subprocess

import numpy as np
import pytest

import tree_fuzz as tf
from test_cpp_host_example import _read_pfm, exe  # noqa: F401  (the fixture that compiles the example)
from test_gpu_textures import _write_images

pytestmark = pytest.mark.gpu
SEED = 36      # random_scene(36, objects=0, twins=False): the first of the tie-free seeds


def test_hprt_render_builds_the_bvhold_tree(exe, tmp_path):  # noqa: F811
    _write_images(tmp_path)
    text = (tf.random_scene(SEED, objects=0, twins=False) % {"dir": str(tmp_path)}).replace("WorldBegin", "Accelerator $acc\nWorldBegin", 1)
    images, errs = {}, {}
    for name, acc in (("bvh", '"bvh"'), ("bvhold", '"bvhold" "string splitmethod" "hlbvh"')):
        p = tmp_path / (name + ".pbrt")
        p.write_text(text.replace("$acc", acc))
        out = str(tmp_path / (name + ".pfm"))
        r = subprocess.run([exe, str(p), out], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        images[name], errs[name] = _read_pfm(out), r.stderr
    assert "hprt_bvhold_build" in errs["bvhold"] and '"bvh" used' not in errs["bvhold"]
    assert "hprt_bvhold_build" not in errs["bvh"]
    assert images["bvh"][..., :3].max() > 0
    assert np.array_equal(images["bvh"].view(np.uint32), images["bvhold"].view(np.uint32))
