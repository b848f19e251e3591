"""Integrator "directlighting" on the GPU: hprt_render_direct and hprt_sample_direct against the test-side restatement of the
reference's direct-lighting render (tests/dl_reference.cpp, held on the CPU by tests/test_dl_host.py) — the film's xyz and weight
sums, the radiance of single samples and the ray counts, bit for bit and number for number.  Films are 32 x 32 pixels or smaller at
2 or 3 samples per pixel; the restated render of each case is computed once and shared."""
import os

import numpy as np
import pytest

import bsdf_cases as bc
import dl_ref
import tree_fuzz as tf
import tree_ref
from test_gpu_ao import _WALKS, _config
from test_gpu_scenes import BUMPY, CASES, FLOOR, MATTE, PLASTIC
from test_host_side import _write_pfm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
STRATEGIES = ("all", "one")
DEPTHS = (1, 2, 5)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _window(opt, x0, y0, w=32, h=32, spp=2):
    """a copy of opt cropped to about w x h pixels at (x0, y0)"""
    o = opt.copy()
    o.crop[0], o.crop[1] = max(0.0, (x0 - 0.5) / o.xres), min(1.0, (x0 + w - 0.5) / o.xres)
    o.crop[2], o.crop[3] = max(0.0, (y0 - 0.5) / o.yres), min(1.0, (y0 + h - 0.5) / o.yres)
    o.spp = spp
    bx0, by0, bx1, by1 = o.film_bounds()
    assert 0 < bx1 - bx0 <= w + 1 and 0 < by1 - by0 <= h + 1
    return o


class _Case:
    """A scene on the device and under the restatement, with the film options of the case and its lights' sample counts"""

    def __init__(self, hprt, path, opt=None, model=None, counts=None):
        self.hprt, self.path = hprt, path
        self.model = model or hprt.Model.load(path)
        self.opt = opt or self.model.options.copy()
        self.counts = list(self.model.direct()[2]) if counts is None else list(counts)
        self.scene = hprt.Scene(self.model, hprt.Bvh(self.model))
        self.ref = dl_ref.DlScene(path)
        self.ref.set_options(self.opt)
        assert self.ref.n_lights == len(self.counts) == self.model.counts()["lights"]
        self._films = {}

    def restated(self, strategy, depth, counts=None):
        counts = self.counts if counts is None else list(counts)
        key = (strategy, depth, tuple(counts))
        if key not in self._films:
            film, c, L = self.ref.render(strategy, depth, counts)
            film.setflags(write=False)
            self._films[key] = (film, c)
        return self._films[key]

    def check(self, strategy, depth, what="", counts=None, **kw):
        """the device film and ray counts equal the restatement's; returns (film, stats, restated counters)"""
        counts = self.counts if counts is None else list(counts)
        film0, c0 = self.restated(strategy, depth, counts)
        film1, st = self.scene.render_direct(strategy, depth, counts, opt=self.opt, **kw)
        what = "%s %s maxdepth %d %s %s" % (os.path.basename(self.path), strategy, depth, counts, what)
        bad = int((_bits(film0) != _bits(film1)).any(-1).sum())
        assert bad == 0, "%s: %d of %d pixels differ" % (what, bad, film0.shape[0] * film0.shape[1])
        for k in ("camera_rays", "rays", "shadow_rays"):
            assert st[k] == c0[k], (what, k, st[k], c0[k])
        return film1, st, c0

    def check_samples(self, strategy, depth, count=128, seed=0, counts=None):
        """hprt_sample_direct on random samples of the sample bounds, numbers beyond the film's spp among them"""
        counts = self.counts if counts is None else list(counts)
        rng = np.random.default_rng(seed)
        _, (sx0, sy0, sx1, sy1) = self.ref.bounds()
        px = rng.integers(sx0, sx1, count).astype(np.int32); py = rng.integers(sy0, sy1, count).astype(np.int32)
        s = rng.integers(0, 5, count).astype(np.int64)
        L0 = self.ref.sample(px, py, s, strategy, depth, counts)
        L1 = self.scene.sample_direct(px, py, s, strategy, depth, counts, opt=self.opt)
        bad = np.flatnonzero((_bits(L0) != _bits(L1)).any(-1))
        assert bad.size == 0, (self.path, strategy, depth, bad.size, L0[bad[:4]].tolist(), L1[bad[:4]].tolist())
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


def _scene(body, eye=(0, -6, 3.5), look=(0, 0, 0.3), res=32, spp=2, extra="", film="", fov=40):
    return ('LookAt %r %r %r  %r %r %r  0 0 1\nCamera "perspective" "float fov" [%r]\nFilm "image" "integer xresolution" [%d] "integer yresolution" [%d] %s\n'
            'Sampler "halton" "integer pixelsamples" [%d] %s\nIntegrator "directlighting"\nWorldBegin\n%s\nWorldEnd\n'
            % (*[float(v) for v in eye], *[float(v) for v in look], float(fov), res, res, film, spp, extra, body))


# ---- the main sweep: two scenes x two strategies x three depths x six light sets ----
def _light_sets(c, e):
    """light sets around a scene centred at c of extent e; %(dir)s: where hdr.pfm lies"""
    def at(dx, dy, dz):
        return "%r %r %r" % (float(c[0] + dx * e), float(c[1] + dy * e), float(c[2] + dz * e))
    sphere = ('AttributeBegin\nMaterial "matte" "color Kd" [0 0 0]\nTranslate %s\nAreaLightSource "diffuse" "color L" [40 38 30] "integer nsamples" [%%d]\n'
              'Shape "sphere" "float radius" [%r]\nAttributeEnd\n' % (at(0.9, -0.2, 1.1), 0.12 * e))

    def tri(dz, flip, two):
        p = np.array([[-0.5, -0.5, dz], [0.5, -0.5, dz], [0.0, 0.6, dz]]) * e + np.asarray(c)
        if flip:
            p = p[::-1]
        return ('AttributeBegin\nMaterial "matte" "color Kd" [0 0 0]\nAreaLightSource "diffuse" "color L" [9 8 7] "integer samples" [2]%s\n%s\nAttributeEnd\n'
                % (' "bool twosided" ["true"]' if two else "", _mesh(p.reshape(1, 9))))
    return {
        "point": 'LightSource "point" "point from" [%s] "color I" [%r %r %r]\n' % (at(0.8, -0.9, 1.2), 3 * e * e, 3 * e * e, 2.5 * e * e),
        "distant": 'LightSource "distant" "point from" [1 -1 3] "point to" [0 0 0] "color L" [2 2 1.5]\n',
        "sphere": sphere % 2,
        # two one-triangle emitters above the scene, the first facing down, the second facing up and two-sided
        "triangles": tri(1.3, True, False) + tri(1.5, False, True),
        "infinite": ('LightSource "infinite" "rgb L" [.4 .45 .5] "integer nsamples" [2]\n'
                     'AttributeBegin\nRotate -90 1 0 0\nRotate 40 0 0 1\nLightSource "infinite" "string mapname" "%(dir)s/hdr.pfm" "integer samples" [3]\nAttributeEnd\n'),
        "mix": ('LightSource "point" "point from" [%s] "color I" [%r %r %r]\n' % (at(-0.8, -0.9, 1.0), e * e, 2 * e * e, 3 * e * e) + sphere % 3 +
                'LightSource "infinite" "rgb L" [.2 .25 .3] "integer nsamples" [4]\n'),
    }


LIGHT_SETS = ("point", "distant", "sphere", "triangles", "infinite", "mix")
EXPECTED_COUNTS = {"point": [1], "distant": [1], "sphere": [2], "triangles": [2, 2], "infinite": [2, 3], "mix": [1, 3, 4]}


def _solid(name):
    """(triangles [n, 9], material line): the dodecahedron (a reflective uber surface: Kd, Ks and Kr, so that maxdepth matters) and the
    first 2,000 triangles of killeroo-simple (matte)"""
    if name == "dodecahedron":
        p9 = tree_ref.BspScene(os.path.join(GOLDEN, "dodecahedron.hprt"), build=False).triangles()
        return p9, 'Material "uber" "color Kd" [.4 .3 .2] "color Ks" [.2 .2 .2] "color Kr" [.3 .3 .4] "float roughness" [.1]\n'
    p9 = tree_ref.BspScene(os.path.join(GOLDEN, "killeroo_simple.hprt"), build=False).triangles()[:2000]
    return p9, 'Material "matte" "color Kd" [.6 .5 .3]\n'


@pytest.fixture(scope="module")
def sweep_cases(hprt, tmp_path_factory):
    d = tmp_path_factory.mktemp("dl_sweep")
    _write_pfm(str(d / "hdr.pfm"), (np.random.default_rng(11).random((33, 57, 3)) * 1.5).astype(np.float32))
    cases = {}

    def get(solid, lights):
        if (solid, lights) not in cases:
            p9, material = _solid(solid)
            lo, hi = p9.reshape(-1, 3).min(0), p9.reshape(-1, 3).max(0)
            c, e = (lo + hi) / 2, float((hi - lo).max())
            body = _light_sets(c, e)[lights] % {"dir": str(d)} + material + _mesh(p9)
            m, path = _bake(hprt, d, "%s_%s" % (solid, lights), _scene(body, eye=c + np.array([1.4 * e, 0.5 * e, 0.6 * e]), look=c))
            assert m.direct()[2] == EXPECTED_COUNTS[lights]
            cases[(solid, lights)] = _Case(hprt, path, model=m)
        return cases[(solid, lights)]
    return get


@pytest.mark.parametrize("lights", LIGHT_SETS)
@pytest.mark.parametrize("solid", ["dodecahedron", "killeroo_prefix"])
def test_film_samples_and_counts_equal_the_restatement(sweep_cases, solid, lights):
    case = sweep_cases(solid, lights)
    for strategy in STRATEGIES:
        for depth in DEPTHS:
            _, st, c0 = case.check(strategy, depth)
            assert 0 < c0["rays"] - c0["camera_rays"] or lights in ("point", "distant")      # BSDF-sampled rays where a light has an area
            assert 0 < c0["shadow_rays"]
            L = case.check_samples(strategy, depth, count=96)
            assert (L > 0).any()
            if solid == "dodecahedron":
                assert (c0["nodes_deep"] > 0) == (depth > 1)      # the uber surface reflects
            else:
                assert c0["nodes_deep"] == 0


# ---- branching: a tree, not a path ----
PANES = "".join('Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-2 -2 %r  2 -2 %r  2 2 %r  -2 2 %r]\n' % ((z,) * 4) for z in (0.6, 1.1, 1.6))
BRANCHING = ('LightSource "point" "point from" [1 -2 4] "color I" [30 30 30]\n'
             'AttributeBegin\nMaterial "matte" "color Kd" [0 0 0]\nTranslate -1.5 -1 3\nAreaLightSource "diffuse" "color L" [20 19 15] "integer nsamples" [2]\n'
             'Shape "sphere" "float radius" [0.35]\nAttributeEnd\n' +
             MATTE + 'Shape "trianglemesh" ' + FLOOR + "\n"
             'Material "uber" "color Kd" [.3 .2 .1] "color Ks" [.1 .1 .1] "color Kr" [.4 .4 .4] "color Kt" [.5 .5 .6] "color opacity" [.5 .5 .5] "float index" [1.3]\n' + PANES +
             'Material "mirror" "color Kr" [.8 .8 .8]\nShape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-2 2 -.4  2 2 -.4  2 2.5 3  -2 2.5 3]\n')


@pytest.fixture(scope="module")
def branching(hprt, tmp_path_factory):
    m, path = _bake(hprt, tmp_path_factory.mktemp("dl_branch"), "branching", _scene(BRANCHING))
    assert m.direct()[2] == [1, 2]
    return _Case(hprt, path, model=m)


@pytest.mark.parametrize("depth", [3, 5])
def test_uber_panes_branch_and_run_out_of_arrays(branching, depth):
    """three uber panes (Kr, Kt, opacity 0.5: a reflection lobe and two transmission lobes) over a matte floor, beside a mirror: the walk
    is a tree whose nodes beyond the first maxdepth find the sample arrays used up (core/integrator.cpp:67-72)"""
    for strategy in STRATEGIES:
        _, st, c0 = branching.check(strategy, depth)
        n_samples = c0["camera_rays"]
        assert 10 * c0["samples_deep2"] >= n_samples, (c0["samples_deep2"], n_samples)      # a node at depth >= 2 under a tenth of the samples at least
        if strategy == "all":
            assert c0["fallback_nodes"] >= 1
        assert c0["nodes_deep"] > n_samples      # more nodes below the camera rays than camera rays: branches
        branching.check_samples(strategy, depth, count=96)


# ---- existing ground ----
def test_smooth_glass_recurses_and_rough_glass_does_not(hprt, tmp_path_factory):
    d = tmp_path_factory.mktemp("dl_glass")
    for name, counts_deep in (("glass", True), ("rough_glass", False)):
        text = CASES[name].replace('Integrator "path"', 'Integrator "directlighting"')
        m, path = _bake(hprt, d, name, text)
        case = _Case(hprt, path, _window(m.options, 20, 30), m)
        for strategy in STRATEGIES:
            _, st, c0 = case.check(strategy, 3)
            assert (c0["nodes_deep"] > 0) == counts_deep
        case.check_samples("all", 3, count=96)


def test_the_sample_number_is_the_pixels_not_the_batchs(hprt, sweep_cases):
    """spp 3 in batches of one sample per pixel against one batch: a batch-local sample number would draw every batch's array samples
    from sample 0's"""
    case = sweep_cases("killeroo_prefix", "mix")
    opt = case.opt.copy()
    opt.spp = 3
    case.ref.set_options(opt)
    try:
        film0, c0, _ = case.ref.render("all", 2, case.counts)
    finally:
        case.ref.set_options(case.opt)
    whole, st0 = case.scene.render_direct("all", 2, case.counts, opt=opt, spp_chunk=0)
    cut, st1 = case.scene.render_direct("all", 2, case.counts, opt=opt, spp_chunk=1)
    assert np.array_equal(_bits(whole), _bits(cut)) and np.array_equal(_bits(whole), _bits(film0))
    for st in (st0, st1):
        assert (st["camera_rays"], st["rays"], st["shadow_rays"]) == (c0["camera_rays"], c0["rays"], c0["shadow_rays"])


def test_hit_ranges_through_a_small_ray_buffer(hprt, sweep_cases, branching):
    """a buffer of 100 light samples: the hits of a step go through the traces in ranges of 14 (seven samples per hit) or 33"""
    was = hprt.debug_dl_ray_capacity(100)
    try:
        case = sweep_cases("killeroo_prefix", "mix")      # counts 1, 3, 4: eight items per hit
        _, st, c0 = case.check("all", 2, "(100-item buffer)")
        assert st["occluded_launches"] > 4
        _, st, c0 = branching.check("all", 3, "(100-item buffer)")
        assert st["occluded_launches"] > 4
        branching.check("one", 3, "(100-item buffer)")
    finally:
        hprt.debug_dl_ray_capacity(was)


def test_crop_window_pixel_centres_and_tile_shards(hprt, tmp_path_factory):
    """a crop window whose sample bounds start at (37, 21), samplepixelcenter, and the two tile shards (0, 2) and (1, 2), whose buffers
    sum to the full film"""
    text = CASES["odd_resolution_crop"].replace('Sampler "halton"', 'Sampler "halton" "bool samplepixelcenter" ["true"]').replace('Integrator "path"', 'Integrator "directlighting"')
    m, path = _bake(hprt, tmp_path_factory.mktemp("dl"), "crop", text)
    opt = m.options.copy()
    opt.crop[0], opt.crop[1], opt.crop[2], opt.crop[3] = 36.5 / 131, 65.5 / 131, 20.5 / 77, 49.5 / 77
    opt.spp = 3
    case = _Case(hprt, path, opt, m, counts=[3])
    assert opt.sample_pixel_center == 1 and case.ref.bounds()[1][:2] == [37, 21]
    full, st, c0 = case.check("all", 2)
    parts = [case.scene.render_direct("all", 2, [3], opt=opt, tile_begin=b, tile_stride=2) for b in (1, 0)]
    assert all(p[0][..., 3].any() for p in parts)
    assert np.array_equal(_bits(parts[0][0] + parts[1][0]), _bits(full))
    assert sum(p[1]["shadow_rays"] for p in parts) == st["shadow_rays"] and sum(p[1]["rays"] for p in parts) == st["rays"]
    for b, p in zip((1, 0), parts):
        ref_part, _, _ = case.ref.render("all", 2, [3], tile_begin=b, tile_stride=2)
        assert np.array_equal(_bits(ref_part), _bits(p[0]))
    case.check_samples("all", 2)


def test_object_instances_transform_the_interaction(hprt):
    path = os.path.join(GOLDEN, "simple_instanced.hprt")
    m = hprt.Model.load(path)
    assert m.counts()["spheres"] == 8 and m.counts()["lights"] >= 1
    case = _Case(hprt, path, _window(m.options, 334, 334), m)
    for strategy in STRATEGIES:
        _, st, c0 = case.check(strategy, 3, counts=[2] * len(case.counts))
        assert 0 < c0["shadow_rays"]
    case.check_samples("all", 3, counts=[2] * len(case.counts))


def test_shading_normals_under_reverse_orientation(hprt, tmp_path_factory):
    text = CASES["reverse_orientation_scaled"].replace('Integrator "path"', 'Integrator "directlighting"')
    m, path = _bake(hprt, tmp_path_factory.mktemp("dl"), "normals", text)
    case = _Case(hprt, path, _window(m.options, 32, 24), m, counts=[3])
    for strategy in STRATEGIES:
        _, st, c0 = case.check(strategy, 2)
        assert 0 < c0["shadow_rays"]
    case.check_samples("all", 2)


def test_camera_rays_that_partly_miss_under_a_mapped_infinite_light(hprt, tmp_path_factory):
    d = tmp_path_factory.mktemp("dl_env")
    _write_pfm(str(d / "hdr.pfm"), (np.random.default_rng(11).random((33, 57, 3)) * 1.5).astype(np.float32))
    body = ('AttributeBegin\nRotate -90 1 0 0\nRotate 40 0 0 1\nLightSource "infinite" "string mapname" "%s/hdr.pfm" "integer nsamples" [2]\nAttributeEnd\n' % d +
            PLASTIC + 'Shape "trianglemesh" ' + BUMPY + '\nAttributeBegin\nMaterial "mirror"\nTranslate 1.2 .4 .6\nShape "sphere" "float radius" [.45]\nAttributeEnd\n')
    m, path = _bake(hprt, d, "env", _scene(body))
    case = _Case(hprt, path, model=m)
    for strategy in STRATEGIES:
        film, st, c0 = case.check(strategy, 3)
        assert c0["nodes_deep"] > 0
    # some camera rays hit (they queue light samples), some escape (they carry the map's radiance)
    L = case.check_samples("all", 3)
    assert 0 < c0["shadow_rays"] < 2 * c0["camera_rays"] and (L > 0).all()


def test_a_textured_kd_at_maxdepth_one(hprt, tmp_path_factory):
    """an image texture on Kd, filtered with the camera ray's differentials — beside a mirror, which maxdepth 1 never leaves"""
    d = tmp_path_factory.mktemp("dl_tex")
    bc.write_checks_pfm(str(d / "checks.pfm"))
    body = ('LightSource "point" "point from" [1 -2 4] "color I" [30 30 30]\nLightSource "infinite" "rgb L" [.2 .2 .3] "integer nsamples" [2]\n'
            'Texture "checks" "spectrum" "imagemap" "string filename" "%s/checks.pfm" "float uscale" [3] "float vscale" [3]\n' % d +
            'Material "matte" "texture Kd" "checks"\nShape "trianglemesh" ' + FLOOR + "\n" + 'Material "mirror"\nShape "trianglemesh" ' + BUMPY + "\n")
    m, path = _bake(hprt, d, "textured", _scene(body))
    case = _Case(hprt, path, model=m)
    for strategy in STRATEGIES:
        film, st, c0 = case.check(strategy, 1)
        assert c0["nodes_deep"] == 0 and film[..., :3].max() > 0
    case.check_samples("all", 1)
    with pytest.raises(hprt.HprtError) as e:      # the mirror's child would meet the texture without the reference's differentials
        case.scene.render_direct("all", 2, case.counts, opt=case.opt)
    assert e.value.code == hprt.E_UNSUPPORTED and "ray differentials" in str(e.value)
    with pytest.raises(hprt.HprtError) as e:
        case.scene.sample_direct([3], [3], [0], "one", 2, case.counts, opt=case.opt)
    assert e.value.code == hprt.E_UNSUPPORTED


def test_a_shadow_grid_scene_takes_the_walk(hprt, tmp_path_factory):
    """one point light, triangles only: the path render's shadow rays take the light-centred grid, these never do"""
    m, path = _bake(hprt, tmp_path_factory.mktemp("dl"), "point_light", CASES["point_light"])
    case = _Case(hprt, path, _window(m.options, 30, 20), m)
    info = case.scene.shadow_grid_info()
    assert info["eligible"]
    case.check("all", 2)
    case.check("one", 2)
    assert case.scene.shadow_grid_info()["render_launches"] == info["render_launches"] == 0
    case.scene.render(case.opt)
    assert case.scene.shadow_grid_info()["render_launches"] > 0      # (the grid is in use for what it is for)


# ---- workspace and ordering ----
def test_count_work_counters_equal_the_restatements(hprt, sweep_cases, branching):
    """(scenes without triangle emitters: the tests inside Shape::Pdf are no traversal's)"""
    for case, depth in ((sweep_cases("dodecahedron", "mix"), 2), (sweep_cases("killeroo_prefix", "sphere"), 1), (branching, 3)):
        plain, _, c0 = case.check("all", depth)
        counted, st, _ = case.check("all", depth, "(counting)", count_work=True)
        assert np.array_equal(_bits(plain), _bits(counted))
        for k in ("nodes_fetched", "nodes_entered", "tri_tests", "sphere_tests", "nodes_fetched_p", "nodes_entered_p", "tri_tests_p", "sphere_tests_p"):
            assert st[k] == c0[k], (case.path, k, st[k], c0[k])
        assert st["nodes_entered_p"] > 0 and st["tri_tests_p"] > 0


def test_a_poisoned_workspace_changes_nothing(hprt, branching):
    branching.scene.debug_poison(0xFF)
    try:
        for strategy in STRATEGIES:
            branching.check(strategy, 3, "(poisoned)")
        branching.check_samples("all", 3)
    finally:
        branching.scene.debug_poison(None)


def test_path_and_ao_renders_before_and_after_are_equal(hprt, branching):
    sc, opt = branching.scene, branching.opt
    before, st0 = sc.render(opt)
    ao_before, sa0 = sc.render_ao(5, True, opt)
    branching.check("all", 3)
    branching.check("one", 3)
    after, st1 = sc.render(opt)
    ao_after, sa1 = sc.render_ao(5, True, opt)
    assert np.array_equal(_bits(before), _bits(after)) and before[..., :3].max() > 0
    assert np.array_equal(_bits(ao_before), _bits(ao_after)) and ao_before[..., :3].max() > 0
    assert (st0["rays"], st0["shadow_rays"]) == (st1["rays"], st1["shadow_rays"])
    assert (sa0["rays"], sa0["shadow_rays"]) == (sa1["rays"], sa1["shadow_rays"])


def test_refusals_on_a_scene(hprt, branching):
    sc, opt = branching.scene, branching.opt
    refused = [
        (dict(max_depth=0), hprt.E_INVALID), (dict(n_light_samples=[1, 0]), hprt.E_INVALID),
        (dict(n_light_samples=[1]), hprt.E_INVALID), (dict(n_light_samples=[1, 2, 3]), hprt.E_INVALID), (dict(n_light_samples=None, n_lights=3), hprt.E_INVALID),
        (dict(max_depth=hprt.DIRECT_MAX_DEPTH + 1), hprt.E_UNSUPPORTED),
        (dict(strategy="one", max_depth=8), hprt.E_UNSUPPORTED),                 # 5 + 5 * 255 + 4 * 127 dimensions
        (dict(max_depth=7), hprt.E_UNSUPPORTED),                                 # "all", two lights: 5 + 56 + 8 * 120 + 4 * 63
        (dict(n_light_samples=[1, 70000]), hprt.E_UNSUPPORTED),
        (dict(flags=hprt.RENDER_PIXEL_STATS), hprt.E_UNSUPPORTED), (dict(flags=hprt.RENDER_EXPORT_FOREIGN), hprt.E_UNSUPPORTED),
    ]
    for kw, code in refused:
        args = dict(strategy="all", max_depth=3, n_light_samples=[1, 2], opt=opt)
        args.update(kw)
        with pytest.raises(hprt.HprtError) as e:
            sc.render_direct(**args)
        assert e.value.code == code and str(e.value), (kw, e.value.code, str(e.value))
    big = opt.copy()
    big.spp = 1 << 21
    with pytest.raises(hprt.HprtError) as e:
        sc.render_direct("all", 1, [1, 1024], opt=big)
    assert e.value.code == hprt.E_UNSUPPORTED and "INT32_MAX" in str(e.value)
    assert sc.render_direct("all", 1, None, opt=opt)[0][..., :3].max() > 0      # no counts: every light once
    branching.check("all", 3, "(after the refusals)")


# ---- every tree walk ----
@pytest.mark.parametrize("name", _WALKS)
def test_every_walk_gives_the_bvhs_film(hprt, tmp_path_factory, name):
    """a tie-free random scene (tests/tree_fuzz.py): through the attached tree the film and the ray counts are the BVH's and the
    restatement's"""
    c = _config(name)
    seed = c.film[0]
    m, path = tf.bake(hprt, tmp_path_factory.mktemp("dl_walk"), c.text(seed), "%s_%d" % (name, seed))
    o = m.options
    n_lights = m.counts()["lights"]
    assert n_lights >= 1
    case = _Case(hprt, path, _window(o, max(0, (o.xres - 32) // 2), max(0, (o.yres - 32) // 2)), m, counts=[2] * n_lights)
    # maxdepth 2 — unless the random scene mixes image textures and specular lobes, which hprt_render_direct refuses beyond maxdepth 1
    depth = 2
    try:
        case.scene.render_direct("all", depth, case.counts, opt=case.opt)
    except hprt.HprtError as e:
        assert e.code == hprt.E_UNSUPPORTED and "ray differentials" in str(e)
        depth = 1
    bvh_film, st0, c0 = case.check("all", depth, "(BVH)")
    assert 0 < c0["shadow_rays"]
    tree = c.make(hprt, m)
    getattr(case.scene, c.attach)(tree)
    tree_film, st1, _ = case.check("all", depth, "(%s)" % name)
    assert np.array_equal(_bits(bvh_film), _bits(tree_film))
    assert (st0["camera_rays"], st0["rays"], st0["shadow_rays"]) == (st1["camera_rays"], st1["rays"], st1["shadow_rays"])
    counted, st2, _ = case.check("all", depth, "(%s, counting)" % name, count_work=True)
    assert st2["nodes_entered_p"] > 0 and st2["nodes_entered"] > 0
    case.check("one", depth, "(%s)" % name)
    case.check_samples("all", depth, count=64)
