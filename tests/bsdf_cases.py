"""What tests/test_bsdf_cases_host.py and tests/test_gpu_bsdf.py share: a palette scene with one small triangle per material (the shape
index names the material on both sides), and the (frame, wo, wi, u) queries at which a BSDF can go wrong, in families.

Directions are built in the local shading frame in float32 and carried to the world by the frame; the families that need exact
local values use the identity frame (ss = x, ts = y, ns = ng = z), where the BSDF's to_local is exact.  All u lie in [0, 1); every
direction and frame vector is finite with a length within 1e-3 of 1, except the deliberately non-unit shading.dpdu of the `frames`
family (length in [0.25, 4]) and the wi of the `refract` family's zero-half-vector queries (length 1 / eta: wo + eta * wi == 0 has
no other solution)."""
import numpy as np

f32 = np.float32
ONE_MINUS_EPS = f32(np.nextafter(f32(1), f32(0)))
DIFFUSE, GLOSSY_R, GLOSSY_T, SPECULAR_R, SPECULAR_T = 1 | 4, 1 | 8, 2 | 8, 1 | 16, 2 | 16      # BxDFType values a sample reports
SENTINEL_PDF = f32(-7.0)
FAMILIES = ("random", "grazing", "normal", "pairs", "refract", "u_edges", "frames")
CLASSES = ("matte", "plastic", "mirror", "substrate", "metal", "glass", "roughglass", "uber")


class Entry:
    """One palette material.  mtype: the material type (0 matte, 1 plastic, 2 mirror, 3 substrate, 4 metal, 5 glass, 6 uber) and
    ncomp: the number of non-specular lobes — both written down by hand from the reference's materials/*.cpp, not read back.
    types: every BxDFType a Sample_f(BSDF_ALL) can report.  eta: the index the refract family aims with.  dead: the material has a
    refraction that can fail (pdf == 0, sampledType == 0).  smooth: one FresnelSpecular lobe that reflects totally from inside."""

    def __init__(self, name, cls, text, mtype, ncomp, types, eta=1.5, dead=False, smooth=False):
        self.name, self.cls, self.text, self.mtype, self.ncomp, self.types = name, cls, text, mtype, ncomp, frozenset(types)
        self.eta, self.dead, self.smooth = f32(eta), dead, smooth

    @property
    def has_lobe(self):
        return bool(self.types)


def _m(kind, *params):
    return 'Material "%s" %s' % (kind, " ".join(params))


def _c(name, r, g, b):
    return '"color %s" [%g %g %g]' % (name, r, g, b)


def _f(name, v):
    return '"float %s" [%g]' % (name, v)


def _b(name, v):
    return '"bool %s" ["%s"]' % (name, "true" if v else "false")


E = Entry
PALETTE = [
    # ---- matte (materials/matte.cpp:45-62): Lambertian, or OrenNayar when Clamp(sigma, 0, 90) != 0; a black Kd adds no lobe
    E("matte", "matte", _m("matte", _c("Kd", .5, .4, .3)), 0, 1, {DIFFUSE}),
    E("matte_black", "matte", _m("matte", _c("Kd", 0, 0, 0)), 0, 0, ()),
    E("matte_clamped_kd", "matte", _m("matte", _c("Kd", -.5, 1.7, .4)), 0, 1, {DIFFUSE}),
    E("matte_sigma0", "matte", _m("matte", _c("Kd", .6, .6, .2), _f("sigma", 0)), 0, 1, {DIFFUSE}),
    E("matte_sigma35", "matte", _m("matte", _c("Kd", .5, .4, .3), _f("sigma", 35)), 0, 1, {DIFFUSE}),
    E("matte_sigma90", "matte", _m("matte", _c("Kd", .5, .4, .3), _f("sigma", 90)), 0, 1, {DIFFUSE}),
    E("matte_sigma120", "matte", _m("matte", _c("Kd", .2, .4, .3), _f("sigma", 120)), 0, 1, {DIFFUSE}),
    E("matte_sigma_neg", "matte", _m("matte", _c("Kd", .2, .7, .3), _f("sigma", -5)), 0, 1, {DIFFUSE}),
    # ---- plastic (materials/plastic.cpp:45-70): Lambertian, then MicrofacetReflection with FresnelDielectric(1.5, 1)
    E("plastic_ks_black", "plastic", _m("plastic", _c("Kd", .4, .5, .6), _c("Ks", 0, 0, 0)), 1, 1, {DIFFUSE}),
    E("plastic_kd_black", "plastic", _m("plastic", _c("Kd", 0, 0, 0), _c("Ks", .4, .5, .6), _f("roughness", .1)), 1, 1, {GLOSSY_R}),
    E("plastic_r0", "plastic", _m("plastic", _c("Kd", .4, .5, .6), _c("Ks", .3, .3, .3), _f("roughness", 0)), 1, 2, {DIFFUSE, GLOSSY_R}),
    E("plastic_r001", "plastic", _m("plastic", _c("Kd", .4, .5, .6), _c("Ks", .3, .3, .3), _f("roughness", .001)), 1, 2, {DIFFUSE, GLOSSY_R}),
    E("plastic_r08", "plastic", _m("plastic", _c("Kd", .4, .5, .6), _c("Ks", .3, .3, .3), _f("roughness", .08)), 1, 2, {DIFFUSE, GLOSSY_R}),
    E("plastic_r1", "plastic", _m("plastic", _c("Kd", .4, .5, .6), _c("Ks", .3, .3, .3), _f("roughness", 1)), 1, 2, {DIFFUSE, GLOSSY_R}),
    E("plastic_noremap", "plastic", _m("plastic", _c("Kd", .4, .5, .6), _c("Ks", .3, .3, .3), _f("roughness", .08), _b("remaproughness", False)), 1, 2,
      {DIFFUSE, GLOSSY_R}),
    # ---- mirror (materials/mirror.cpp:44-56): SpecularReflection with FresnelNoOp
    E("mirror", "mirror", _m("mirror", _c("Kr", .9, .8, .7)), 2, 0, {SPECULAR_R}),
    E("mirror_black", "mirror", _m("mirror", _c("Kr", 0, 0, 0)), 2, 0, ()),
    # ---- substrate (materials/substrate.cpp:44-65): one FresnelBlend lobe unless both reflectances are black
    E("substrate", "substrate", _m("substrate", _c("Kd", .5, .3, .2), _c("Ks", .2, .2, .3), _f("uroughness", .1), _f("vroughness", .1)), 3, 1, {GLOSSY_R}),
    E("substrate_aniso", "substrate", _m("substrate", _c("Kd", .5, .3, .2), _c("Ks", .2, .2, .3), _f("uroughness", .5), _f("vroughness", .002)), 3, 1,
      {GLOSSY_R}),
    E("substrate_kd_black", "substrate", _m("substrate", _c("Kd", 0, 0, 0), _c("Ks", .2, .2, .3)), 3, 1, {GLOSSY_R}),
    E("substrate_ks_black", "substrate", _m("substrate", _c("Kd", .5, .3, .2), _c("Ks", 0, 0, 0), _b("remaproughness", False)), 3, 1, {GLOSSY_R}),
    E("substrate_black", "substrate", _m("substrate", _c("Kd", 0, 0, 0), _c("Ks", 0, 0, 0)), 3, 0, ()),
    # ---- metal (materials/metal.cpp:59-79): one conductor MicrofacetReflection lobe, always
    E("metal_gold_r001", "metal", _m("metal", _c("eta", .143, .375, 1.442), _c("k", 3.983, 2.386, 1.603), _f("roughness", .001)), 4, 1, {GLOSSY_R}),
    E("metal_gold_r05", "metal", _m("metal", _c("eta", .143, .375, 1.442), _c("k", 3.983, 2.386, 1.603), _f("roughness", .05)), 4, 1, {GLOSSY_R}),
    E("metal_alu_r5", "metal", _m("metal", _c("eta", 1.657, .880, .521), _c("k", 9.224, 6.270, 4.837), _f("roughness", .5)), 4, 1, {GLOSSY_R}),
    E("metal_aniso", "metal", _m("metal", _c("eta", 1.657, .880, .521), _c("k", 9.224, 6.270, 4.837), _f("uroughness", .3), _f("vroughness", .02),
                                 _b("remaproughness", False)), 4, 1, {GLOSSY_R}),
    # ---- smooth glass (materials/glass.cpp:44-65, allowMultipleLobes): one FresnelSpecular lobe unless R and T are both black
    E("glass_15", "glass", _m("glass", _f("index", 1.5)), 5, 0, {SPECULAR_R, SPECULAR_T}, eta=1.5, smooth=True),
    E("glass_133", "glass", _m("glass", _c("Kr", .9, 1, .8), _c("Kt", .7, .8, .9), _f("index", 1.33)), 5, 0, {SPECULAR_R, SPECULAR_T}, eta=1.33, smooth=True),
    E("glass_1", "glass", _m("glass", _f("index", 1)), 5, 0, {SPECULAR_R, SPECULAR_T}, eta=1),      # (FrDielectric(c, 1, 1) is 0 up to rounding — and 1 where the sine rounds to 1: the grazing family reflects)
    E("glass_kr_black", "glass", _m("glass", _c("Kr", 0, 0, 0), _f("index", 1.5)), 5, 0, {SPECULAR_R, SPECULAR_T}, eta=1.5, smooth=True),
    # (index 3: reflection, the only live sample here, is then the likelier one over the sphere of wo)
    E("glass_kt_black", "glass", _m("glass", _c("Kt", 0, 0, 0), _f("index", 3)), 5, 0, {SPECULAR_R, SPECULAR_T}, eta=3, smooth=True),
    E("glass_black", "glass", _m("glass", _c("Kr", 0, 0, 0), _c("Kt", 0, 0, 0)), 5, 0, ()),
    # ---- rough glass (materials/glass.cpp:66-93): MicrofacetReflection and / or MicrofacetTransmission over one distribution
    E("roughglass", "roughglass", _m("glass", _f("uroughness", .2), _f("vroughness", .2)), 5, 2, {GLOSSY_R, GLOSSY_T}, dead=True),
    E("roughglass_r_only", "roughglass", _m("glass", _c("Kt", 0, 0, 0), _f("uroughness", .3), _f("vroughness", .1)), 5, 1, {GLOSSY_R}),
    E("roughglass_t_only", "roughglass", _m("glass", _c("Kr", 0, 0, 0), _f("uroughness", .3), _f("vroughness", .1)), 5, 1, {GLOSSY_T}, dead=True),
    E("roughglass_u0", "roughglass", _m("glass", _f("uroughness", 0), _f("vroughness", .25)), 5, 2, {GLOSSY_R, GLOSSY_T}, dead=True),
    E("roughglass_noremap", "roughglass", _m("glass", _f("uroughness", .2), _f("vroughness", .35), _f("index", 1.33), _b("remaproughness", False)), 5, 2,
      {GLOSSY_R, GLOSSY_T}, eta=1.33, dead=True),
    # ---- uber (materials/uber.cpp:45-108): [1 - opacity straight through], Lambertian, microfacet, [Kr], [Kt]
    E("uber_all", "uber", _m("uber", _c("Kd", .4, .3, .2), _c("Ks", .3, .3, .4), _c("Kr", .2, .3, .2), _c("Kt", .5, .4, .5), _c("opacity", .7, .7, .7),
                             _f("index", 1.5)), 6, 2, {SPECULAR_T, DIFFUSE, GLOSSY_R, SPECULAR_R}, dead=True),
    E("uber_opaque", "uber", _m("uber", _c("Kd", .4, .3, .2), _c("Ks", .3, .3, .4), _f("index", 1.4), _f("uroughness", .2), _f("vroughness", .05)), 6, 2,
      {DIFFUSE, GLOSSY_R}, eta=1.4),
    E("uber_clear", "uber", _m("uber", _c("Kd", .4, .3, .2), _c("Ks", .3, .3, .4), _c("Kr", .2, .3, .2), _c("Kt", .5, .4, .5), _c("opacity", 0, 0, 0)), 6, 0,
      {SPECULAR_T}),
    E("uber_kr_behind", "uber", _m("uber", _c("Kd", .4, .3, .2), _c("Ks", .3, .3, .4), _c("Kr", .2, .3, .2)), 6, 2, {DIFFUSE, GLOSSY_R, SPECULAR_R}),
    E("uber_kt_only", "uber", _m("uber", _c("Kd", 0, 0, 0), _c("Ks", 0, 0, 0), _c("Kt", .5, .4, .5)), 6, 0, {SPECULAR_T}, dead=True),
    E("uber_kr_kt", "uber", _m("uber", _c("Kd", 0, 0, 0), _c("Ks", 0, 0, 0), _c("Kr", .2, .3, .2), _c("Kt", .5, .4, .5), _f("index", 1.33)), 6, 0,
      {SPECULAR_R, SPECULAR_T}, eta=1.33, dead=True),
    E("uber_index1", "uber", _m("uber", _c("Kd", .5, .5, .5), _c("Ks", .25, .25, .25), _c("Kr", .1, .1, .1), _c("Kt", .1, .1, .1), _c("opacity", .9, .8, .7),
                                _f("index", 1), _b("remaproughness", False)), 6, 2, {SPECULAR_T, DIFFUSE, GLOSSY_R, SPECULAR_R}, eta=1),
]
del E
NAMES = [e.name for e in PALETTE]
assert len(set(NAMES)) == len(NAMES) and {e.cls for e in PALETTE} == set(CLASSES)


def palette_pbrt():
    """The palette as one .pbrt text: shape k is a small triangle of PALETTE[k]'s material."""
    head = ('LookAt 0 0 5  0 0 0  0 1 0\nCamera "perspective" "float fov" [40]\nFilm "image" "integer xresolution" [8] "integer yresolution" [8]\n'
            'Sampler "halton" "integer pixelsamples" [1]\nIntegrator "path"\nWorldBegin\nLightSource "point" "point from" [0 0 4] "color I" [5 5 5]\n')
    body = []
    for k, e in enumerate(PALETTE):
        x = .1 * k
        body.append('AttributeBegin\n%s\nShape "trianglemesh" "integer indices" [0 1 2] "point P" [%g 0 0  %g 0 0  %g .05 0]\nAttributeEnd\n'
                    % (e.text, x, x + .05, x))
    return head + "".join(body) + "WorldEnd\n"


# one triangle whose Kd is an image texture: what the probe refuses (the 2 x 2 PFM is written beside the scene)
TEXTURED_PBRT = ('LookAt 0 0 5  0 0 0  0 1 0\nCamera "perspective" "float fov" [40]\nFilm "image" "integer xresolution" [8] "integer yresolution" [8]\n'
                 'Sampler "halton" "integer pixelsamples" [1]\nIntegrator "path"\nWorldBegin\nLightSource "point" "point from" [0 0 4] "color I" [5 5 5]\n'
                 'Texture "checks" "spectrum" "imagemap" "string filename" "%(dir)s/checks.pfm"\nMaterial "matte" "texture Kd" "checks"\n'
                 'Shape "trianglemesh" "integer indices" [0 1 2] "point P" [0 0 0  1 0 0  0 1 0] "float uv" [0 0 1 0 0 1]\nWorldEnd\n')


def build_palette(hprt, orc, directory):
    """(model, oracle scene) of the palette: the front end parses the text, the baked container goes to the oracle, the model to
    hprt.Scene — both hold the shapes in creation order"""
    p = directory / "palette.pbrt"
    p.write_text(palette_pbrt())
    model = hprt.Model.parse(str(p))
    assert model.warnings() == [], model.warnings()
    baked = str(directory / "palette.hprt")
    model.save(baked)
    return model, orc.OracleScene(baked)


def write_checks_pfm(path):
    texels = np.array([[[.8, .2, .2], [.2, .8, .2]], [[.2, .2, .8], [.7, .7, .7]]], "<f4")
    with open(path, "wb") as f:
        f.write(b"PF\n2 2\n-1.0\n" + texels.tobytes())


# ---- building blocks (everything float32) ----

def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(f32)


def sphere_dirs(rng, n):
    return _unit(rng.normal(size=(n, 3)))


def _with_z(rng, z):
    """unit float32 vectors whose z component is exactly z (|z| <= 1): the other two components carry the rest at a random azimuth"""
    z = np.asarray(z, f32)
    phi = rng.uniform(0, 2 * np.pi, z.shape[0])
    s = np.sqrt(np.maximum(0.0, 1.0 - z.astype(np.float64) ** 2))
    return np.stack([(s * np.cos(phi)).astype(f32), (s * np.sin(phi)).astype(f32), z], axis=1)


IDENTITY = np.array([0, 0, 1, 0, 0, 1, 1, 0, 0], f32)      # n, shading.n, shading.dpdu


def identity_frames(n):
    return np.tile(IDENTITY, (n, 1))


def random_frames(rng, n):
    """orthonormal: ng = ns random, dpdu a random unit vector orthogonal to it"""
    ns = sphere_dirs(rng, n).astype(np.float64)
    t = rng.normal(size=(n, 3))
    t -= ns * np.sum(t * ns, axis=1, keepdims=True)
    ss = _unit(t)
    ns = ns.astype(f32)
    return np.concatenate([ns, ns, ss], axis=1)


def frame_axes(frame9):
    """(ss, ts, ns) as the BSDF forms them: ss = Normalize(dpdu), ts = Cross(ns, ss), in float32 operations"""
    ns, d = frame9[:, 3:6], frame9[:, 6:9]
    ss = (d / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).astype(f32))[:, None]).astype(f32)
    ts = np.cross(ns.astype(np.float64), ss.astype(np.float64)).astype(f32)
    return ss, ts, ns


def to_world(frame9, local):
    ss, ts, ns = frame_axes(frame9)
    return (ss * local[:, 0:1] + ts * local[:, 1:2] + ns * local[:, 2:3]).astype(f32)


def refract(wo, eta):
    """Refract(wo, Faceforward((0, 0, 1), wo), eta) in float32 operations (core/reflection.h:96-108); rows where it fails get -wo"""
    n = np.where(wo[:, 2:3] < 0, f32(-1), f32(1)) * np.array([0, 0, 1], f32)
    eta = f32(eta)
    cos_i = (n[:, 2] * wo[:, 2]).astype(f32)
    sin2_i = np.maximum(f32(0), (f32(1) - cos_i * cos_i).astype(f32))
    sin2_t = (eta * eta * sin2_i).astype(f32)
    ok = sin2_t < 1
    cos_t = np.sqrt(np.where(ok, f32(1) - sin2_t, f32(0)).astype(f32))
    wt = (eta * -wo + ((eta * cos_i - cos_t).astype(f32))[:, None] * n).astype(f32)
    return np.where(ok[:, None], wt, -wo).astype(f32), ok


def _neighbours(v):
    v = f32(v)
    return [np.nextafter(v, f32(0)), v, np.nextafter(v, f32(2))]


U0_EDGES = sorted({float(x) for x in [f32(0), ONE_MINUS_EPS] + [y for m in range(2, 6) for k in range(1, m) for y in _neighbours(f32(k) / f32(m))]})
U1_EDGES = sorted({float(x) for x in [f32(0), ONE_MINUS_EPS] + _neighbours(.5)})
GRAZING_Z = np.array([0.0, -0.0] + [s * 2.0 ** -k for k in range(10, 150) for s in (1, -1)], f32)
assert np.all(np.array(U0_EDGES + U1_EDGES) < 1) and GRAZING_Z.size == 282 and np.count_nonzero(GRAZING_Z) == 280


# ---- the families: each returns (frame9, wo, wi, u) ----

def fam_random(rng, e, n=2048):
    fr = random_frames(rng, n)
    return fr, sphere_dirs(rng, n), sphere_dirs(rng, n), rng.random((n, 2), f32)


def fam_grazing(rng, e):
    """wo.z and / or wi.z in {+-0, +-2^-k, k = 10..149} exactly (identity frame); 128 more with wo.z = +-0 and a free wi"""
    z = GRAZING_Z
    n = z.size
    wo = np.concatenate([_with_z(rng, z), sphere_dirs(rng, n), _with_z(rng, z), _with_z(rng, np.tile(np.array([0.0, -0.0], f32), 64))])
    wi = np.concatenate([sphere_dirs(rng, n), _with_z(rng, z), _with_z(rng, rng.permutation(z)), sphere_dirs(rng, 128)])
    return identity_frames(wo.shape[0]), wo, wi, rng.random((wo.shape[0], 2), f32)


def fam_normal(rng, e):
    """wo = (0, 0, +-1); a fine sweep of the polar angle (tan theta from 1e-4 to 1e4, both hemispheres): TrowbridgeReitzSample11's
    cosTheta > .9999 branch is taken after the stretch by alpha, so every alpha of the palette has its threshold somewhere in the
    sweep; z right around .9999; and the few float32 z next to 1, whose sine is 0 or just above OrenNayar's 1e-4"""
    pole = np.array([[0, 0, 1], [0, 0, -1]] * 32, f32)
    tan = np.exp(rng.uniform(np.log(1e-4), np.log(1e4), 1024))
    sweep = _with_z(rng, (1.0 / np.sqrt(1.0 + tan * tan)) * rng.choice([-1.0, 1.0], tan.size))
    near = _with_z(rng, rng.uniform(.9998, 1.0, 256) * rng.choice([-1.0, 1.0], 256))
    one = f32(1)
    zs = [one]
    for _ in range(7):
        zs.append(np.nextafter(zs[-1], f32(0)))
    tiny = _with_z(rng, np.array(zs * 16, f32) * rng.choice([-1.0, 1.0], 128).astype(f32))
    a = np.concatenate([pole, sweep, near, tiny])
    n = a.shape[0]
    # the special direction as wo with a free wi, as wi with a free wo, and both special
    wo = np.concatenate([a, sphere_dirs(rng, n), a])
    wi = np.concatenate([sphere_dirs(rng, n), a, a[rng.permutation(n)]])
    return identity_frames(3 * n), wo, wi, rng.random((3 * n, 2), f32)


def fam_pairs(rng, e, n=256):
    """wi the mirror image of wo (wh is the normal), wi = -wo (zero half vector), wi = wo"""
    wo = np.concatenate([sphere_dirs(rng, n - 2), np.array([[0, 0, 1], [0, 0, -1]], f32)])
    wos = np.concatenate([wo, wo, wo])
    wis = np.concatenate([wo * np.array([-1, -1, 1], f32), -wo, wo])
    return identity_frames(3 * n), wos, wis, rng.random((3 * n, 2), f32)


def fam_refract(rng, e, n=256):
    """from outside and from inside (wo.z < 0), away from, next to and beyond the critical angle sin theta = 1 / eta: wi =
    Refract(wo, +-z, eta), wi = Refract(wo, +-z, 1 / eta), and wi with wo + eta' * wi == 0 exactly (eta' = eta for wo.z > 0, 1 / eta
    below: the half vector of MicrofacetTransmission is Normalize(0), so NaN is expected there)"""
    eta = e.eta
    crit = min(1.0, 1.0 / float(eta)) if eta != 1 else 1.0
    s = np.concatenate([rng.uniform(0, 1, n), np.clip(crit + rng.uniform(-2e-3, 2e-3, n), 0, 1), np.clip(crit * (1 + rng.uniform(-3e-7, 3e-7, n // 2)), 0, 1),
                        rng.uniform(crit, 1, n // 2)])
    sign = np.where(np.arange(s.size) % 4 == 0, 1.0, -1.0)      # three in four from inside, where total internal reflection lives
    wo = _with_z(rng, np.sqrt(np.maximum(0.0, 1.0 - s * s)) * sign)
    wo = wo[wo[:, 2] != 0]
    inv = f32(1) / eta
    wi_a, _ = refract(wo, eta)
    wi_b, _ = refract(wo, inv)
    # wo + eta' * wi == 0: wi = -wo / eta' cut to 12 mantissa bits, then wo := -(wi * eta') in float32 — the product the BSDF forms
    ep = np.where(wo[:, 2:3] > 0, eta, inv).astype(f32)
    wi_c = (-(wo / ep)).astype(f32)
    wi_c = (wi_c.view(np.uint32) & np.uint32(0xFFFFF000)).view(f32)
    wo_c = (-(wi_c * ep)).astype(f32)
    assert np.all((wo_c + wi_c * ep).astype(f32) == 0)
    keep = wo_c[:, 2] != 0
    wo_c, wi_c = wo_c[keep], wi_c[keep]
    wos = np.concatenate([wo, wo, wo_c])
    wis = np.concatenate([wi_a, wi_b, wi_c])
    return identity_frames(wos.shape[0]), wos, wis, rng.random((wos.shape[0], 2), f32)


def fam_u_edges(rng, e, per=4):
    """u0 in {0, OneMinusEpsilon, k / m and both float neighbours for m = 2..5}, u1 in {0, .5 and neighbours, OneMinusEpsilon},
    crossed, each pair with `per` random directions; for smooth glass 4,096 evenly spaced u0 more, so that u0 < F falls on both
    sides at many F"""
    u0, u1 = np.meshgrid(np.array(U0_EDGES, f32), np.array(U1_EDGES, f32), indexing="ij")
    u = np.repeat(np.stack([u0.ravel(), u1.ravel()], axis=1), per, axis=0)
    if e.mtype == 5 and e.ncomp == 0:
        even = (np.arange(4096, dtype=np.float64) / 4096).astype(f32)
        u = np.concatenate([u, np.stack([even, rng.random(4096, f32)], axis=1)])
    n = u.shape[0]
    return random_frames(rng, n), sphere_dirs(rng, n), sphere_dirs(rng, n), u.astype(f32)


def fam_frames(rng, e, n=1024):
    """shading normal tilted from the geometric one by up to 89 degrees, the geometric normal flipped in half of them, shading.dpdu
    neither unit (length in [0.25, 4]) nor orthogonal to the shading normal (up to about 30 degrees off), as interpolated normals give;
    half of the directions near the geometric normal's horizon, where dot(w, ng) and the local z differ in sign"""
    ng = sphere_dirs(rng, n).astype(np.float64)
    t = rng.normal(size=(n, 3))
    t -= ng * np.sum(t * ng, axis=1, keepdims=True)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    tilt = np.radians(rng.uniform(0, 89, n))[:, None]
    ns = np.cos(tilt) * ng + np.sin(tilt) * t
    b = np.cross(ns, rng.normal(size=(n, 3)))
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    dpdu = (b + ns * rng.uniform(-.6, .6, n)[:, None])
    dpdu *= (rng.uniform(.25, 4, n) / np.linalg.norm(dpdu, axis=1))[:, None]
    ng = np.where((np.arange(n) % 2 == 0)[:, None], ng, -ng)
    fr = np.concatenate([ng.astype(f32), _unit(ns), dpdu.astype(f32)], axis=1)

    def dirs():
        w = rng.normal(size=(n, 3))
        h = w - ng * np.sum(w * ng, axis=1, keepdims=True)      # in the geometric horizon, then lifted off it by up to +-0.5 rad
        h /= np.linalg.norm(h, axis=1, keepdims=True)
        lift = rng.uniform(-.5, .5, n)[:, None]
        near = np.cos(lift) * h + np.sin(lift) * ng
        return _unit(np.where((np.arange(n) % 4 < 2)[:, None], near, w))
    return fr, dirs(), dirs(), rng.random((n, 2), f32)


_FAMILY_FN = {"random": fam_random, "grazing": fam_grazing, "normal": fam_normal, "pairs": fam_pairs, "refract": fam_refract, "u_edges": fam_u_edges,
              "frames": fam_frames}


def queries(entries=None, seed=7):
    """All families for the given palette entries (default: all).  Returns a dict of arrays over the queries: shape int32, family int8
    (index into FAMILIES), frame9, wo, wi (world) and u."""
    out = {k: [] for k in ("shape", "family", "frame9", "wo", "wi", "u")}
    for k, e in enumerate(PALETTE):
        if entries is not None and e.name not in entries:
            continue
        for fi, fam in enumerate(FAMILIES):
            rng = np.random.default_rng([seed, k, fi])
            fr, wo, wi, u = _FAMILY_FN[fam](rng, e)
            n = fr.shape[0]
            assert n > 0 and wo.shape == (n, 3) and wi.shape == (n, 3) and u.shape == (n, 2)
            assert all(a.dtype == f32 for a in (fr, wo, wi, u))
            out["shape"].append(np.full(n, k, np.int32)); out["family"].append(np.full(n, fi, np.int8))
            if fam != "frames":      # (the frames family builds world directions: its frames are not orthonormal)
                wo, wi = to_world(fr, wo), to_world(fr, wi)
            out["frame9"].append(fr); out["wo"].append(wo); out["wi"].append(wi); out["u"].append(u)
    return {k: np.concatenate(v) for k, v in out.items()}


def by_class(cls):
    return [e.name for e in PALETTE if e.cls == cls]


def compare(got, want):
    """Bit identity of two [n, 8] float32 arrays, NaN compared as a class: where `want` is NaN `got` must be NaN (any sign, any
    payload — the default NaN of x86 and of gfx950 differ), everywhere else the words must be equal.  Returns (bad rows, number
    of NaN-against-NaN words)."""
    g, w = got.view(np.uint32), want.view(np.uint32)
    wn, gn = np.isnan(want), np.isnan(got)
    ok = np.where(wn, gn, g == w)
    return np.flatnonzero(~ok.all(axis=1)), int((wn & gn).sum())
