"""Accelerator "kdtree" where the kd walk does not apply or a tree is refused: scenes with object instances keep the BVH and
today's warning (model, library and the C++ host example agree); trees deeper than the walk's todo list are refused; the
structural check that guards hprt_scene_attach_kdtree rejects every malformed tree."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

INSTANCED_KD = """LookAt 3 4 1.5  .5 .5 0  0 0 1
Camera "perspective" "float fov" [45]
Film "image" "integer xresolution" [64] "integer yresolution" [48]
Sampler "halton" "integer pixelsamples" [4]
Integrator "path" "integer maxdepth" [3]
Accelerator "kdtree"
WorldBegin
LightSource "point" "point from" [0 0 5] "color I" [10 10 10]
ObjectBegin "tri"
Shape "trianglemesh" "integer indices" [0 1 2] "point P" [0 0 0 1 0 0 0 1 0]
ObjectEnd
AttributeBegin
Translate .2 .1 0
ObjectInstance "tri"
AttributeEnd
ObjectInstance "tri"
Shape "trianglemesh" "integer indices" [0 1 2 2 3 0] "point P" [-2 -2 -.1 2 -2 -.1 2 2 -.1 -2 2 -.1]
WorldEnd
"""
KD = INSTANCED_KD.replace('ObjectBegin "tri"\n', "").replace("ObjectEnd\n", "").replace('ObjectInstance "tri"\n', "")


def _parse(hprt, tmp_path, text, name):
    p = tmp_path / name
    p.write_text(text)
    return hprt.Model.parse(str(p)), str(p)


def test_instanced_kdtree_scene_keeps_the_bvh_and_its_warning(hprt, tmp_path):
    m, _ = _parse(hprt, tmp_path, INSTANCED_KD, "inst.pbrt")
    assert m.accelerator == "kdtree"
    w = m.warnings()
    assert 'Accelerator "kdtree" is outside the hot-path scope; "bvh" used' in w, w
    assert not any("hprt_scene_attach_kdtree" in x for x in w), w
    with pytest.raises(hprt.HprtError) as e:
        hprt.KdTree(m)
    assert e.value.code == hprt.E_UNSUPPORTED
    hprt.Bvh(m)                                     # the BVH the scene keeps
    m2, _ = _parse(hprt, tmp_path, KD, "kd.pbrt")
    assert any("hprt_scene_attach_kdtree" in x for x in m2.warnings()) and not any("outside the hot-path scope" in x for x in m2.warnings())
    assert hprt.KdTree(m2).info()["nodes"] >= 1


def test_trees_deeper_than_the_todo_list_are_refused(hprt):
    """100,000 points with a full empty bonus: every empty-space cut is free, so the tree goes 73 levels deep when maxdepth lets it."""
    rng = np.random.default_rng(1)
    p = rng.uniform(0, 1, (100000, 3)).astype(np.float32)
    with pytest.raises(hprt.HprtError) as e:
        hprt.KdTree.from_bounds(p, p, empty_bonus=1.0, max_depth=300)
    assert e.value.code == hprt.E_UNSUPPORTED and "deeper than" in str(e.value)
    ok = hprt.KdTree.from_bounds(p, p, empty_bonus=1.0, max_depth=hprt.KD_MAX_DEPTH)
    assert 60 <= ok.info()["depth"] <= hprt.KD_MAX_DEPTH


CHECK_DRIVER = r"""
#include <cstdio>
#include <cstring>
#include "kdtree_builder.h"
using namespace hprt;
static int fails = 0;
static void expect(const KdTree &t, const char *want, uint32_t depth = 0) {
    uint32_t d = 12345;
    const char *got = CheckKdTree(t, &d);
    if (std::strstr(got, want) == nullptr || (!*want && d != depth)) { std::printf("want '%s' got '%s' depth %u\n", want, got, d); ++fails; }
}
static KdNode leaf(uint32_t np, uint32_t a) { return KdNode{a, 3u | (np << 2)}; }
static KdNode interior(uint32_t axis, uint32_t above) { return KdNode{0x3f800000u, axis | (above << 2)}; }
int main() {
    KdTree t; t.nPrims = 3;
    t.nodes = {interior(0, 2), leaf(1, 0), leaf(2, 0)}; t.primIndices = {1, 2};
    expect(t, "", 1);                                                           // well-formed, one interior level
    KdTree e = t; e.nodes.clear(); expect(e, "no nodes");
    e = t; e.nodes = {interior(0, 2)}; expect(e, "no below child");
    e = t; e.nodes[0] = interior(1, 1); expect(e, "above child is out of range");   // the above child cannot be the below child
    e = t; e.nodes[0] = interior(1, 3); expect(e, "above child is out of range");   // past the end
    e = t; e.nodes[1] = leaf(1, 3); expect(e, "one-primitive leaf");
    e = t; e.nodes[2] = leaf(2, 1); expect(e, "runs past primitiveIndices");
    e = t; e.primIndices = {1, 7}; expect(e, "primitiveIndices names");
    return fails;
}
"""


def test_attach_check_rejects_malformed_trees(tmp_path):
    """CheckKdTree (csrc/kdtree_builder.cpp) is what hprt_scene_attach_kdtree applies before anything reaches the device; the
    builders cannot produce a malformed tree, so it is driven here directly, built from the library's own source."""
    src = tmp_path / "check.cpp"
    src.write_text(CHECK_DRIVER)
    csrc = os.path.join(ROOT, "thesis-pbrt-v3_amd", "csrc")
    exe = str(tmp_path / "check")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + csrc, str(src), os.path.join(csrc, "kdtree_builder.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout


@pytest.fixture(scope="module")
def example(hprt, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cppkd") / "hprt_render")
    lib = os.path.join(ROOT, "thesis-pbrt-v3_amd", "lib")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "hprt_render.cpp"), "-o", out, "-L" + lib, "-lhprt", "-Wl,-rpath," + lib],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def _read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF"
        w, h = [int(v) for v in f.readline().split()]
        scale = float(f.readline())
        data = np.frombuffer(f.read(), "<f4" if scale < 0 else ">f4").reshape(h, w, 3)
    return data[::-1].astype(np.float32)


@pytest.mark.gpu
def test_example_renders_instanced_kdtree_scenes_with_the_bvh(hprt, example, tmp_path):
    """examples/hprt_render.cpp on a kdtree scene with object instances: it renders (with the BVH, as before the kd walk existed)
    and reports the model's warning; its image is the BVH render's."""
    m, path = _parse(hprt, tmp_path, INSTANCED_KD, "inst.pbrt")
    out = str(tmp_path / "inst.pfm")
    r = subprocess.run([example, path, out, "--spp", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert '"bvh" used' in r.stderr
    opt = m.options.copy(); opt.spp = 2
    film, _ = hprt.Scene(m, hprt.Bvh(m), device=0).render(opt)
    assert np.array_equal(_read_pfm(out).view(np.uint32), hprt.film_resolve(film, opt.film_scale).view(np.uint32))


@pytest.mark.gpu
def test_example_attaches_the_kdtree(hprt, example, tmp_path):
    m, path = _parse(hprt, tmp_path, KD, "kd.pbrt")
    out = str(tmp_path / "kd.pfm")
    r = subprocess.run([example, path, out, "--spp", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    opt = m.options.copy(); opt.spp = 2
    sc = hprt.Scene(m, hprt.Bvh(m), device=0)
    sc.attach_kdtree(hprt.KdTree(m))
    film, _ = sc.render(opt)
    assert np.array_equal(_read_pfm(out).view(np.uint32), hprt.film_resolve(film, opt.film_scale).view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("acc", ["rbsp", "rbspkd"])
def test_example_attaches_the_rbsp_trees(hprt, example, tmp_path, acc):
    """The same for Accelerator "rbsp" and "rbspkd": the example's image is Scene.attach_rbsp / attach_rbspkd + render's."""
    m, path = _parse(hprt, tmp_path, KD.replace('Accelerator "kdtree"', 'Accelerator "%s"' % acc), acc + ".pbrt")
    out = str(tmp_path / (acc + ".pfm"))
    r = subprocess.run([example, path, out, "--spp", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert '"bvh" used' not in r.stderr, r.stderr
    opt = m.options.copy(); opt.spp = 2
    sc = hprt.Scene(m, hprt.Bvh(m), device=0)
    if acc == "rbsp":
        sc.attach_rbsp(hprt.Rbsp(m))
    else:
        sc.attach_rbspkd(hprt.RbspKd(m))
    film, _ = sc.render(opt)
    assert np.array_equal(_read_pfm(out).view(np.uint32), hprt.film_resolve(film, opt.film_scale).view(np.uint32))
