"""Integrator "ambientocclusion" on the GPU: hprt_render_ao and hprt_sample_ao against the test-side restatement of the reference's
ambient-occlusion render (tests/ao_reference.cpp, held on the CPU by tests/test_ao_host.py) — the film's xyz and weight sums, the
radiance of single samples and the ray counts, bit for bit and number for number.  Films are 32 x 32 pixels or smaller at up to 4
samples per pixel; the restated render of each case is computed once and shared."""
import os

import numpy as np
import pytest

import ao_ref
import tree_fuzz as tf
import tree_ref
from test_gpu_scenes import CASES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
N_SAMPLES = (1, 3, 64, 65, 130)      # one ray; a count that divides nothing; one wave; counts that cross a wave


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _window(opt, x0, y0, w=32, h=32, spp=2):
    """a copy of opt cropped to about w x h pixels at (x0, y0)"""
    o = opt.copy()
    # (half a pixel below each bound: ceil(resolution * crop) in float is then the bound itself)
    o.crop[0], o.crop[1] = max(0.0, (x0 - 0.5) / o.xres), min(1.0, (x0 + w - 0.5) / o.xres)
    o.crop[2], o.crop[3] = max(0.0, (y0 - 0.5) / o.yres), min(1.0, (y0 + h - 0.5) / o.yres)
    o.spp = spp
    bx0, by0, bx1, by1 = o.film_bounds()
    assert 0 < bx1 - bx0 <= w + 1 and 0 < by1 - by0 <= h + 1
    return o


class _Case:
    """A baked scene on the device and under the restatement, with the film options of the case"""

    def __init__(self, hprt, path, opt=None, model=None):
        self.hprt, self.path = hprt, path
        self.model = model or hprt.Model.load(path)
        self.opt = opt or self.model.options.copy()
        self.scene = hprt.Scene(self.model, hprt.Bvh(self.model))
        self.ref = ao_ref.AoScene(path)
        self.ref.set_options(self.opt)
        self._films = {}

    def restated(self, n, cos):
        if (n, cos) not in self._films:
            film, c = self.ref.render(n, cos)
            film.setflags(write=False)
            self._films[(n, cos)] = (film, c)
        return self._films[(n, cos)]

    def check(self, n, cos, what="", **kw):
        """the device film and ray counts of (n, cos) equal the restatement's; returns (film, stats, restated counters)"""
        film0, c0 = self.restated(n, cos)
        film1, st = self.scene.render_ao(n, cos, self.opt, **kw)
        what = "%s n_samples %d %s %s" % (os.path.basename(self.path), n, "cosine" if cos else "uniform", what)
        bad = int((_bits(film0) != _bits(film1)).any(-1).sum())
        assert bad == 0, "%s: %d of %d pixels differ" % (what, bad, film0.shape[0] * film0.shape[1])
        for k in ("camera_rays", "rays", "shadow_rays"):
            assert st[k] == c0[k], (what, k, st[k], c0[k])
        return film1, st, c0

    def check_samples(self, n, cos, count=192, seed=0):
        """hprt_sample_ao on random samples of the sample bounds, numbers beyond the film's spp among them"""
        rng = np.random.default_rng(seed)
        _, (sx0, sy0, sx1, sy1) = self.ref.bounds()
        px = rng.integers(sx0, sx1, count).astype(np.int32); py = rng.integers(sy0, sy1, count).astype(np.int32)
        s = rng.integers(0, 7, count).astype(np.int64)
        L0 = self.ref.sample(px, py, s, n, cos)
        L1 = self.scene.sample_ao(px, py, s, n, cos, self.opt)
        assert np.array_equal(_bits(L0), _bits(L1)), (self.path, n, cos, int((_bits(L0) != _bits(L1)).any(-1).sum()))
        return L0


def _bake(hprt, d, name, text):
    p = d / (name + ".pbrt")
    p.write_text(text)
    m = hprt.Model.parse(str(p))
    path = str(d / (name + ".hprt"))
    m.save(path)
    return m, path


def _mesh(p9):
    return ('Shape "trianglemesh" "integer indices" [' + " ".join(str(i) for i in range(3 * p9.shape[0])) + '] "point P" [' +
            " ".join("%r" % float(v) for v in p9.ravel()) + "]")


@pytest.fixture(scope="module")
def dodecahedron(hprt):
    path = os.path.join(GOLDEN, "dodecahedron.hprt")
    m = hprt.Model.load(path)
    return _Case(hprt, path, _window(m.options, 334, 334), m)


@pytest.fixture(scope="module")
def killeroo_prefix(hprt, tmp_path_factory):
    """the first 2,000 triangles of killeroo-simple in front of a camera of their own, 32 x 32 pixels uncropped"""
    p9 = tree_ref.BspScene(os.path.join(GOLDEN, "killeroo_simple.hprt"), build=False).triangles()[:2000]
    lo, hi = p9.reshape(-1, 3).min(0), p9.reshape(-1, 3).max(0)
    c, e = (lo + hi) / 2, float((hi - lo).max())
    eye = c + np.array([1.4 * e, 0.5 * e, 0.6 * e])
    text = ('LookAt %r %r %r  %r %r %r  0 0 1\nCamera "perspective" "float fov" [40]\nFilm "image" "integer xresolution" [32] "integer yresolution" [32]\n'
            'Sampler "halton" "integer pixelsamples" [2]\nIntegrator "ambientocclusion"\nWorldBegin\nMaterial "matte"\n%s\nWorldEnd\n'
            % (*[float(v) for v in eye], *[float(v) for v in c], _mesh(p9)))
    m, path = _bake(hprt, tmp_path_factory.mktemp("ao"), "killeroo_prefix", text)
    assert m.counts()["triangles"] == 2000
    return _Case(hprt, path, model=m)


@pytest.fixture(scope="module")
def two_scenes(dodecahedron, killeroo_prefix):
    return {"dodecahedron": dodecahedron, "killeroo_prefix": killeroo_prefix}


@pytest.mark.parametrize("cos", [True, False], ids=["cosine", "uniform"])
@pytest.mark.parametrize("n", N_SAMPLES)
@pytest.mark.parametrize("name", ["dodecahedron", "killeroo_prefix"])
def test_film_samples_and_counts_equal_the_restatement(two_scenes, name, n, cos):
    case = two_scenes[name]
    _, st, c0 = case.check(n, cos)
    # camera rays that hit and camera rays that escaped, occluded and open hemisphere rays
    assert 0 < c0["shadow_rays"] and c0["shadow_rays"] % n == 0
    L = case.check_samples(n, cos)
    assert (L > 0).any()


def test_the_sample_number_is_the_pixels_not_the_batchs(hprt, killeroo_prefix):
    """spp 3 in batches of one sample per pixel: a batch-local sample number would draw every batch's array samples from sample 0's"""
    case = killeroo_prefix
    opt = case.opt.copy()
    opt.spp = 3
    case.ref.set_options(opt)
    try:
        film0, c0 = case.ref.render(5, True)
    finally:
        case.ref.set_options(case.opt)
    whole, st0 = case.scene.render_ao(5, True, opt, spp_chunk=0)
    cut, st1 = case.scene.render_ao(5, True, opt, spp_chunk=1)
    assert np.array_equal(_bits(whole), _bits(cut)) and np.array_equal(_bits(whole), _bits(film0))
    for st in (st0, st1):
        assert (st["camera_rays"], st["rays"], st["shadow_rays"]) == (c0["camera_rays"], c0["rays"], c0["shadow_rays"])
    assert st1["extend_launches"] == 3 and st0["extend_launches"] == 1


def test_hit_ranges_through_a_small_ray_buffer(hprt, killeroo_prefix):
    """a ray buffer of 1,000 rays: the hits of a batch go through the any-hit walk in ranges of 7 (n = 130) or 333 (n = 3)"""
    was = hprt.debug_ao_ray_capacity(1000)
    try:
        for n in (130, 3):
            _, st, c0 = killeroo_prefix.check(n, True, "(1,000-ray buffer)")
            assert st["occluded_launches"] == -(-(c0["shadow_rays"] // n) // (1000 // n)) > 1
    finally:
        hprt.debug_ao_ray_capacity(was)


def test_crop_window_pixel_centres_and_tile_shards(hprt, tmp_path_factory):
    """a crop window whose sample bounds start at (37, 21), samplepixelcenter, and the two tile shards (0, 2) and (1, 2), whose buffers
    sum to the full film"""
    text = CASES["odd_resolution_crop"].replace('Sampler "halton"', 'Sampler "halton" "bool samplepixelcenter" ["true"]')
    m, path = _bake(hprt, tmp_path_factory.mktemp("ao"), "crop", text)
    opt = m.options.copy()
    opt.crop[0], opt.crop[1], opt.crop[2], opt.crop[3] = 36.5 / 131, 65.5 / 131, 20.5 / 77, 49.5 / 77
    opt.spp = 3
    case = _Case(hprt, path, opt, m)
    assert opt.sample_pixel_center == 1 and case.ref.bounds()[1][:2] == [37, 21]
    full, st, c0 = case.check(7, False)
    parts = [case.scene.render_ao(7, False, opt, tile_begin=b, tile_stride=2) for b in (1, 0)]
    assert all(p[0][..., 3].any() for p in parts)
    assert np.array_equal(_bits(parts[0][0] + parts[1][0]), _bits(full))
    assert sum(p[1]["shadow_rays"] for p in parts) == st["shadow_rays"] and sum(p[1]["rays"] for p in parts) == st["rays"]
    for b, p in zip((1, 0), parts):
        ref_part, _ = case.ref.render(7, False, tile_begin=b, tile_stride=2)
        assert np.array_equal(_bits(ref_part), _bits(p[0]))
    case.check_samples(7, False)


def test_killeroo_simple_with_its_sphere(hprt):
    path = os.path.join(GOLDEN, "killeroo_simple.hprt")
    m = hprt.Model.load(path)
    assert m.counts()["spheres"] == 1
    case = _Case(hprt, path, _window(m.options, 294, 329), m)      # (the window of the smoke test)
    _, st, c0 = case.check(64, True)
    case.check(17, False)
    case.check_samples(64, True)
    assert 0 < c0["shadow_rays"]


def test_object_instances_transform_the_interaction(hprt):
    path = os.path.join(GOLDEN, "simple_instanced.hprt")
    m = hprt.Model.load(path)
    assert m.counts()["spheres"] == 8
    case = _Case(hprt, path, _window(m.options, 334, 334), m)
    for cos in (True, False):
        _, st, c0 = case.check(16, cos)
        assert 0 < c0["shadow_rays"]
    case.check_samples(16, True)


def test_shading_normals_and_reverse_orientation(hprt, tmp_path_factory):
    """a mesh with normals under ReverseOrientation and a mirroring scale: isect.n is flipped towards the shading normal, and
    Faceforward(isect.n, -ray.d) flips it again for some hits and not for others"""
    xs = np.linspace(-2, 2, 9)
    P = np.array([[x, y, 0.3 * np.sin(1.3 * x) * np.cos(0.9 * y)] for y in xs for x in xs], np.float32)
    N = np.array([[-0.39 * np.cos(1.3 * x) * np.cos(0.9 * y), 0.27 * np.sin(1.3 * x) * np.sin(0.9 * y), 1.0] for y in xs for x in xs], np.float32)
    idx = []
    for j in range(8):
        for i in range(8):
            a = j * 9 + i
            idx += [a, a + 1, a + 10, a, a + 10, a + 9]
    mesh = ('Shape "trianglemesh" "integer indices" [%s] "point P" [%s] "normal N" [%s]'
            % (" ".join(map(str, idx)), " ".join("%r" % float(v) for v in P.ravel()), " ".join("%r" % float(v) for v in N.ravel())))
    text = ('LookAt 0 -6 3.5  0 0 0.3  0 0 1\nCamera "perspective" "float fov" [40]\nFilm "image" "integer xresolution" [32] "integer yresolution" [24]\n'
            'Sampler "halton" "integer pixelsamples" [2]\nIntegrator "ambientocclusion"\nWorldBegin\nMaterial "matte"\n'
            'AttributeBegin\nScale 1 -1 1.5\nReverseOrientation\n%s\nAttributeEnd\n'
            'AttributeBegin\nTranslate 0 0.5 1.2\nRotate 200 1 0 0\nScale .4 .4 .4\n%s\nAttributeEnd\nWorldEnd\n' % (mesh, mesh))
    m, path = _bake(hprt, tmp_path_factory.mktemp("ao"), "normals", text)
    case = _Case(hprt, path, model=m)
    for cos in (True, False):
        _, st, c0 = case.check(9, cos)
        assert 0 < c0["shadow_rays"] < c0["rays"] * 9      # camera rays partly miss
    case.check_samples(9, True)
    # both outcomes of Faceforward(isect.n, -ray.d) occur among the film's hits
    flips = set()
    for px, py in [(x, y) for y in range(1, 24, 2) for x in range(1, 32, 2)]:
        if len(case.ref.rays(px, py, 0, 9, True)[2]):
            flips.add(case.ref.last_flipped)
    assert flips == {True, False}


def test_a_shadow_grid_scene_takes_the_walk(hprt, tmp_path_factory):
    """one point light, triangles only: the path render's shadow rays take the light-centred grid, the hemisphere rays never do"""
    m, path = _bake(hprt, tmp_path_factory.mktemp("ao"), "point_light", CASES["point_light"])
    case = _Case(hprt, path, _window(m.options, 30, 20), m)
    info = case.scene.shadow_grid_info()
    assert info["eligible"]
    case.check(64, True)
    case.check(5, False)
    assert case.scene.shadow_grid_info()["render_launches"] == info["render_launches"] == 0
    case.scene.render(case.opt)
    assert case.scene.shadow_grid_info()["render_launches"] > 0      # (the grid is in use for what it is for)


def test_count_work_counters_equal_the_restatements(hprt, dodecahedron, killeroo_prefix):
    for case in (dodecahedron, killeroo_prefix):
        plain, _, c0 = case.check(65, True)
        counted, st, _ = case.check(65, True, "(counting)", count_work=True)
        assert np.array_equal(_bits(plain), _bits(counted))
        for k in ("nodes_fetched", "nodes_entered", "tri_tests", "sphere_tests", "nodes_fetched_p", "nodes_entered_p", "tri_tests_p", "sphere_tests_p"):
            assert st[k] == c0[k], (case.path, k, st[k], c0[k])
        assert st["nodes_entered_p"] > 0 and st["tri_tests_p"] > 0


def test_a_poisoned_workspace_changes_nothing(hprt, killeroo_prefix):
    killeroo_prefix.scene.debug_poison(0xFF)
    try:
        killeroo_prefix.check(65, False, "(poisoned)")
        killeroo_prefix.check_samples(65, False)
    finally:
        killeroo_prefix.scene.debug_poison(None)


def test_path_renders_before_and_after_are_equal(hprt, dodecahedron):
    sc, opt = dodecahedron.scene, dodecahedron.opt
    before, st0 = sc.render(opt)
    dodecahedron.check(64, True)
    after, st1 = sc.render(opt)
    assert np.array_equal(_bits(before), _bits(after)) and before[..., :3].max() > 0
    assert (st0["rays"], st0["shadow_rays"]) == (st1["rays"], st1["shadow_rays"])


def test_refusals_on_a_scene(hprt, dodecahedron):
    sc, opt = dodecahedron.scene, dodecahedron.opt
    for n, code in ((0, hprt.E_INVALID), (1025, hprt.E_INVALID)):
        with pytest.raises(hprt.HprtError) as e:
            sc.render_ao(n, True, opt)
        assert e.value.code == code
    big = opt.copy()
    big.spp = 1 << 21
    with pytest.raises(hprt.HprtError) as e:
        sc.render_ao(1024, True, big)
    assert e.value.code == hprt.E_UNSUPPORTED
    dodecahedron.check(3, True, "(after the refusals)")


# ---- every tree walk ----
_WALKS = ["kd", "rbsp13", "rbspkd9", "bsppaper", "bsppaperkd", "bsprandom", "kdinst", "rbspinst13", "rbspkdinst9"]


def _config(name):
    if name == "bsprandom":      # the plain node-based form, K = 5 (tests/tree_fuzz.py lists its withkd and fastkd siblings)
        c = tf.CONFIGS["bsppaper"]
        return tf.Config("bsprandom", lambda hprt, m: hprt.bspnode_tree(m, "bsprandom", n_directions=tf.NODE_K, seed=tf.NODE_SEED)[0], "attach_bsppaper",
                         c.restate, film=c.film, ties=c.ties)
    return tf.CONFIGS[name]


@pytest.mark.parametrize("name", _WALKS)
def test_every_walk_gives_the_bvhs_film(hprt, tmp_path_factory, name):
    """a tie-free random scene (tests/tree_fuzz.py): through the attached tree the film and the ray counts are the BVH's and the
    restatement's"""
    c = _config(name)
    seed = c.film[0]
    m, path = tf.bake(hprt, tmp_path_factory.mktemp("ao_walk"), c.text(seed), "%s_%d" % (name, seed))
    o = m.options
    case = _Case(hprt, path, _window(o, max(0, (o.xres - 32) // 2), max(0, (o.yres - 32) // 2)), m)
    n = 17
    bvh_film, st0, c0 = case.check(n, True, "(BVH)")
    assert 0 < c0["shadow_rays"]
    tree = c.make(hprt, m)
    getattr(case.scene, c.attach)(tree)
    tree_film, st1, _ = case.check(n, True, "(%s)" % name)
    assert np.array_equal(_bits(bvh_film), _bits(tree_film))
    assert (st0["camera_rays"], st0["rays"], st0["shadow_rays"]) == (st1["camera_rays"], st1["rays"], st1["shadow_rays"])
    counted, st2, _ = case.check(n, True, "(%s, counting)" % name, count_work=True)
    assert st2["nodes_entered_p"] > 0 and st2["nodes_entered"] > 0
    case.check_samples(n, True, count=64)
