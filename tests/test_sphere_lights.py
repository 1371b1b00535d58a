"""Sphere lights in next-event estimation (docs/SPEC.md §7.1, PT_FLAG_NEXT_EVENT_SPHERES) without a GPU: the scalar checker of
tests/sphere_light_ref/ against the brute-force path tracer of the oracle and against the §7 / §11 checkers it extends, the cone's
numerics against float64, and the flag's plumbing through the header and the bindings.

The checker writes its own joint table, cone sample, MIS weights and accumulation from the spec; it shares only the unchanged pieces
(closest hit, BSDF sample, camera ray, RNG) with oracle/. The device is held to it bit for bit by tests/test_gpu_sphere_lights.py."""
import inspect
import os
import re

import numpy as np
import pytest

import env_checker as ec
import nee_checker as nc
import sphere_light_checker as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 32       # image side
SPP = 2048   # samples per pixel of the statistical tests
Z = 4.0      # the statistical tests' bound, in standard deviations (the rule of tests/test_nee.py)
MEASURED_VARIANCE_RATIO = 3.9   # test 6, unflagged NEE / flagged on the lamp-only Cornell at SPP
ASSERTED_RATIO = 0.5 * MEASURED_VARIANCE_RATIO
# Test 7: the largest relative error of omc, pdf and thit against float64, measured per band of d / r, and 4 x that.
# Near the surface 1 - r^2/d^2 cancels: cosm, and with it omc and the pdf, keep about 24 + log2(1 - r^2/d^2) bits. thit's error is
# relative to the distance to the sphere's centre: near the silhouette the distance to the surface itself is ill-conditioned.
BANDS = ((1.0 + 2.0 ** -10, 1.01), (1.01, 2.0), (2.0, 2.0 ** 20))
MEASURED_OMC = (1.3e-6, 5.0e-7, 2.0e-7)    # of omc and of the pdf, relative
MEASURED_THIT = (9.0e-5, 6.4e-5, 1.1e-5)   # of thit, relative to the distance to the centre (worst at the silhouette, u1 -> 1)
MEASURED_THIT_INNER = (9.7e-5, 6.0e-6, 1.1e-7)     # of thit, relative to thit itself, for u1 <= 0.9: away from the silhouette


def moments(P, pto, sd, flags, env=None, spp=SPP):
    """(per-pixel mean, per-pixel sample variance of one sample's radiance, stats) of the checker at S x S."""
    params = P.make_params(S, S, spp=spp, max_depth=8, streams=1, seed=11)
    img, st, sq = sc.render(pto, pto.Scene(sd), params, env=env, flags=flags, with_sq=True)
    m = img[..., :3].astype(np.float64)
    return m, (sq / spp - m * m) * spp / (spp - 1), st


def max_z(a, b, spp=SPP):
    """Largest |z| of the difference of two independent estimates: over the whole image and over its 8 x 8-pixel blocks, per channel.
    Every pixel takes part."""
    d, v = a[0] - b[0], (a[1] + b[1]) / spp
    zs = [np.abs(d.sum((0, 1))) / np.sqrt(v.sum((0, 1)))]
    for by in range(0, S, 8):
        for bx in range(0, S, 8):
            zs.append(np.abs(d[by:by + 8, bx:bx + 8].sum((0, 1))) / np.sqrt(v[by:by + 8, bx:bx + 8].sum((0, 1))))
    return float(np.max(zs))


CASES = {"lamp": ("lamp", False), "lamp+quad": ("lamp+quad", False), "lamp+quad+map": ("lamp+quad", True), "glass-lamp": ("glass-lamp", False),
         "two-lamps": ("two-lamps", False)}


def case(P, name):
    scene, with_map = CASES[name]
    return sc.scene(P, scene, S, S), (sc.lit_map(P) if with_map else None)


@pytest.fixture(scope="module")
def brute(P, pto):
    """The plain estimator (§5) of each case: the checker without NEE, which on a scene without a map is pto_render bit for bit."""
    out = {}
    for name in CASES:
        sd, env = case(P, name)
        m, v, st = moments(P, pto, sd, 0, env)
        if env is None:
            ref, ost = pto.render(pto.Scene(sd), P.make_params(S, S, spp=SPP, max_depth=8, streams=1, seed=11))
            assert np.array_equal(m, ref[..., :3].astype(np.float64)) and st.ext_rays == ost.rays and st.shadow_rays == 0, name
        out[name] = (m, v)
    return out


# ------------------------------------------------------------------------------------------------------------------------ 1. plumbing
def test_plumbing(P):
    """PT_FLAG_NEXT_EVENT_SPHERES = 512 in the header, the Python binding and the C# binding; make_params takes sphere_lights; the ABI
    version stays 2."""
    N = P.native
    hdr = open(os.path.join(ROOT, "include", "ptrt.h")).read()
    assert re.search(r"PT_FLAG_NEXT_EVENT_SPHERES\s*=\s*512u", hdr)
    assert N.PT_FLAG_NEXT_EVENT_SPHERES == 512
    cs = open(os.path.join(ROOT, "host", "csharp", "PtrtNative.cs")).read()
    assert re.search(r"\bNextEventSpheres\s*=\s*512\b", cs)
    assert "--nee-spheres" in open(os.path.join(ROOT, "host", "cpp", "main.cpp")).read()
    assert inspect.signature(P.make_params).parameters["sphere_lights"].default is False
    assert P.make_params(4, 4, next_event=True, sphere_lights=True).flags == 256 | 512
    assert N.lib.pt_abi_version() == 2


# -------------------------------------------------------------------------------------------------------------- 2. no sphere light
@pytest.mark.parametrize("name", ["C1", "lights-without-the-sphere's-emission", "C1+map"])
def test_without_a_sphere_light_it_is_the_nee_frame(P, pto, name):
    """On a scene without a sphere light the flagged checker is nee_checker / env_checker bit for bit, rays included."""
    sd = P.make_scene(P.native.PT_SCENE_CORNELL, 0, 3, S, S) if name.startswith("C1") else sc.without_sphere_emission(nc.many_lights_scene(P, S, S))
    env = sc.lit_map(P) if name == "C1+map" else None
    params = P.make_params(S, S, spp=8, max_depth=8, streams=2)
    a, sa, _ = sc.render(pto, pto.Scene(sd), params, env=env)
    b, sb, _ = ec.render(pto, pto.Scene(sd), params, env=env, flags=ec.NEE) if env is not None else nc.render(pto, pto.Scene(sd), params)
    assert sa.n_sphere_lights == 0 and sa.n_lights == sb.n_lights > 0
    assert np.array_equal(a, b) and (sa.ext_rays, sa.shadow_rays, sa.paths) == (sb.ext_rays, sb.shadow_rays, sb.paths)


# ------------------------------------------------------------------------------------------------------------------ 3. unflagged stays
@pytest.mark.parametrize("name", ["lamp", "lamp+quad", "lamp+quad+map", "glass-lamp", "lights"])
def test_unflagged_checkers_are_untouched_and_the_paths_are_the_plain_ones(P, pto, name):
    """On scenes with sphere lights: without SPHERES this checker is still nee_checker / env_checker bit for bit, and the flagged
    frame's extension rays are the plain frame's rays."""
    sd, env = (nc.many_lights_scene(P, S, S), None) if name == "lights" else case(P, name)
    params = P.make_params(S, S, spp=8, max_depth=8, streams=2)
    a, sa, _ = sc.render(pto, pto.Scene(sd), params, env=env, flags=sc.NEE)
    b, sb, _ = ec.render(pto, pto.Scene(sd), params, env=env, flags=ec.NEE) if env is not None else nc.render(pto, pto.Scene(sd), params)
    assert np.array_equal(a, b) and (sa.ext_rays, sa.shadow_rays) == (sb.ext_rays, sb.shadow_rays)
    f, sf, _ = sc.render(pto, pto.Scene(sd), params, env=env)
    plain, sp, _ = sc.render(pto, pto.Scene(sd), params, env=env, flags=0)
    assert sf.n_sphere_lights >= 1 and sf.ext_rays == sp.ext_rays and sf.paths == sp.paths and sf.shadow_rays > 0
    assert not np.array_equal(f, a)
    if env is None:
        _, ost = pto.render(pto.Scene(sd), params)
        assert sf.ext_rays == ost.rays


# ---------------------------------------------------------------------------------------------------------------- 4. same expectation
@pytest.mark.parametrize("name", ["lamp", "lamp+quad", "lamp+quad+map", "glass-lamp", "two-lamps"])
def test_flagged_is_unbiased(P, pto, brute, name):
    """The flagged mean equals the brute-force mean within 4 sigma, over the image and over 8 x 8 blocks, every pixel taking part: a
    Cornell box lit only by a lamp, with the ceiling quad too, under a lit map as well (psel = 1/2), with an emissive glass ball (hit
    from inside after refraction: weight 1), and with two lamps of different power. Measured: 2.1, 2.2, 2.2, 1.4, 1.8 sigma."""
    sd, env = case(P, name)
    m, v, st = moments(P, pto, sd, sc.FLAGGED, env)
    assert st.n_sphere_lights >= 1 and st.shadow_rays > 0
    z = max_z((m, v), brute[name])
    print(name, "z", round(z, 2))
    assert z < Z, (name, z)


# ------------------------------------------------------------------------------------------------------------------------ 5. controls
@pytest.mark.parametrize("name,flag", [("lamp", sc.HITS_WEIGHT_1), ("lamp+quad", sc.HITS_WEIGHT_1), ("lamp", sc.AREA_PDF), ("lamp+quad", sc.AREA_PDF),
                                       ("two-lamps", sc.SWAP_PMF), ("lamp+quad+map", sc.NO_PSEL)])
def test_negative_controls_fail(P, pto, brute, name, flag):
    """Test 4 catches the mistakes it is there for, each by at least 3 Z: sphere hits left at weight 1 (the lamp counted twice), the
    uniform-area pdf of the whole sphere where the cone's stands, the pmfs of two lamps swapped, psel dropped. Measured
    (DESIGN.md §9.1): weight 1 112 / 90 sigma, area pdf 332 / 225, swapped pmf 532, no psel 203; at 512 spp already 56 / 45, 168 / 113,
    266 and 101."""
    sd, env = case(P, name)
    m, v, _ = moments(P, pto, sd, sc.FLAGGED | flag, env)
    z = max_z((m, v), brute[name])
    print(name, flag, "z", round(z, 1))
    assert z > 3 * Z, (name, flag, z)


# ------------------------------------------------------------------------------------------------------------------------ 6. variance
def test_variance_is_lower(P, pto):
    """On the lamp-only Cornell at equal spp the flagged checker's per-pixel variance is lower than the unflagged NEE checker's, which
    finds the lamp by hits only. Half the measured ratio (MEASURED_VARIANCE_RATIO) is asserted."""
    sd, _ = case(P, "lamp")
    _, vu, _ = moments(P, pto, sd, sc.NEE)
    _, vf, _ = moments(P, pto, sd, sc.FLAGGED)
    ratio = vu.mean() / vf.mean()
    print("variance ratio", ratio)
    assert ratio >= ASSERTED_RATIO, ratio


# ------------------------------------------------------------------------------------------------------------------------ 7. numerics
def cone64(c, r, o, u1, u2):
    """§7.1 in float64 from the float32 inputs: 1 - sqrt(1 - r^2/d^2), the direction, thit."""
    c, o, r, u1, u2 = np.asarray(c, np.float64), np.asarray(o, np.float64), float(r), float(u1), float(u2)
    oc = c - o
    d2 = oc @ oc
    cosm = np.sqrt(1.0 - r * r / d2)
    omc = r * r / d2 / (1.0 + cosm)  # == 1 - cosm, exactly, and computable in float64 at d / r = 2^20
    z = u1 * omc
    cos_t, sin2 = 1.0 - z, z * (2.0 - z)
    thit = np.sqrt(d2) * cos_t - np.sqrt(max(0.0, r * r - d2 * sin2))
    return dict(omc=omc, pdf=1.0 / (2.0 * np.pi * omc), thit=thit, cosm=cosm, dist=np.sqrt(d2), axis=oc / np.sqrt(d2), cos_t=cos_t)


def numerics_errors():
    """Per band of d / r: the largest relative error of omc, pdf and thit (the latter relative to the distance to the centre), and the
    smallest dot(wl, axis) - cosm, over radii 2^-20 .. 2^10, d / r from 1 + 2^-10 to 2^20, and a grid of (u1, u2)."""
    rng = np.random.default_rng(7)
    out = [dict(omc=0.0, pdf=0.0, thit=0.0, thit_inner=0.0, inside=np.inf, n=0) for _ in BANDS]
    ratios = np.concatenate([1.0 + 2.0 ** np.linspace(-10, 0, 21), 2.0 ** np.linspace(1, 20, 20)])
    for lr in range(-20, 11, 3):
        r = np.float32(2.0 ** lr)
        for q in ratios:
            axis = rng.normal(size=3)
            axis /= np.linalg.norm(axis)
            c = rng.uniform(-1, 1, 3).astype(np.float32) * r
            o = (c.astype(np.float64) - axis * float(r) * q).astype(np.float32)
            oc = c.astype(np.float64) - o.astype(np.float64)
            ratio = np.sqrt(oc @ oc) / float(r)  # the ratio the float32 inputs really have
            band = next((i for i, (lo, hi) in enumerate(BANDS) if lo <= ratio <= hi), None)
            if band is None:
                continue
            for u1, u2 in ((0.0, 0.0), (0.5, 0.25), (0.9, 0.4), (0.999999, 0.7), (np.float32(rng.uniform()), np.float32(rng.uniform()))):
                got, want = sc.cone(c, r, o, u1, u2), cone64(c, r, o, u1, u2)
                assert got is not None, (r, q)
                e = out[band]
                e["n"] += 1
                e["omc"] = max(e["omc"], abs(float(got["omc"]) - want["omc"]) / want["omc"])
                e["pdf"] = max(e["pdf"], abs(float(got["pdf"]) - want["pdf"]) / want["pdf"])
                e["thit"] = max(e["thit"], abs(float(got["thit"]) - want["thit"]) / want["dist"])
                if u1 <= 0.9:
                    e["thit_inner"] = max(e["thit_inner"], abs(float(got["thit"]) - want["thit"]) / want["thit"])
                e["inside"] = min(e["inside"], float(got["wl"].astype(np.float64) @ want["axis"]) - want["cosm"])
                assert np.isfinite([got["omc"], got["pdf"], got["thit"]]).all() and got["thit"] > 0 and abs(np.linalg.norm(got["wl"].astype(np.float64)) - 1) < 1e-6
    return out


def test_cone_numerics_against_float64():
    """omc, pdf and thit hold to their float64 restatement within 4 x the measured error of their band of d / r, from just outside the
    surface to 2^20 radii away, for radii 2^-20 .. 2^10; and every sampled direction lies inside the cone to within that tolerance.
    The naive 1.0f - cosm (NAIVE_OMC) does not: it is 0 from d / r of about 4000 on."""
    errs = numerics_errors()
    for (lo, hi), e, m_omc, m_thit, m_inner in zip(BANDS, errs, MEASURED_OMC, MEASURED_THIT, MEASURED_THIT_INNER):
        print(f"d/r in [{lo:.6g}, {hi:.6g}]: n {e['n']} omc {e['omc']:.3g} pdf {e['pdf']:.3g} thit {e['thit']:.3g} thit (u1 <= 0.9, relative to thit) {e['thit_inner']:.3g} inside {e['inside']:.3g}")
        assert e["n"] > 100
        assert e["omc"] <= 4 * m_omc and e["pdf"] <= 4 * m_omc, (lo, e)
        assert e["thit"] <= 4 * m_thit, (lo, e)
        assert e["thit_inner"] <= 4 * m_inner, (lo, e)
        assert e["inside"] >= -4 * m_omc, (lo, e)  # dot(wl, axis) >= cosm
    far = sc.cone((0, 0, 0), 1.0, (0, 0, 10000.0), 0.5, 0.5, flags=sc.NAIVE_OMC)
    assert far["omc"] == 0.0 and sc.cone((0, 0, 0), 1.0, (0, 0, 10000.0), 0.5, 0.5)["omc"] > 0


# ---------------------------------------------------------------------------------------------------------------------- 8. finiteness
def test_degenerate_lamps_stay_finite(P, pto):
    """A lamp within ray_eps of the floor, one tangent to a wall, a receiver inside a lamp, two overlapping lamps and a lamp of radius
    2^-20: frames and squared sums are finite, with ray_eps 1e-4 and 0."""
    e, k = (6.0, 6.0, 6.0), (0.5, 0.5, 0.5)
    lamps = (((0.2, -1.0 + 0.1 + 5e-5, 0.3, 0.1), k, e, sc.LAMBERT),                 # within ray_eps of the floor
             ((-1.0 + 0.2, 0.0, 0.0, 0.2), k, e, sc.LAMBERT),                       # tangent to the left wall
             ((0.0, -1.0, -0.5, 0.4), k, e, sc.LAMBERT),                            # the floor passes through it: receivers inside
             ((0.5, 0.3, -0.4, 0.2), k, e, sc.LAMBERT), ((0.6, 0.35, -0.4, 0.2), k, e, sc.LAMBERT),  # overlapping
             ((-0.3, 0.5, 0.2, 2.0 ** -20), k, (1e9, 1e9, 1e9), sc.LAMBERT))          # a point-like lamp
    sd = sc.cornell(P, S, S, lamps=lamps)
    for eps in (1e-4, 0.0):
        params = P.make_params(S, S, spp=64, max_depth=8, streams=2, ray_eps=eps)
        img, st, sq = sc.render(pto, pto.Scene(sd), params, with_sq=True)
        assert st.n_sphere_lights == 6 and st.shadow_rays > 0
        assert np.isfinite(img).all() and np.isfinite(sq).all(), eps


def test_a_distant_lamp_still_contributes(P, pto):
    """A lamp about 100 radii from the receivers: the flagged mean equals brute force at 4 sigma over the image. (Brute force finds a
    lamp d / r away once in (d / r)^2 samples per vertex: 10^4 radii would take 10^10 samples for a hundred hits, so that distance is held to
    the closed form in the next test; the blocks of this one see too few brute-force hits for a variance and take no part.)"""
    lamp = ((0.0, 0.3, 0.0, 0.01), (0.0, 0.0, 0.0), (3e4, 3e4, 3e4), sc.LAMBERT)
    sd = sc.cornell(P, S, S, lamps=(lamp,), quad=False)
    spp = 16384
    params = P.make_params(S, S, spp=spp, max_depth=3, streams=1, seed=3)

    def mom(flags):
        img, st, sq = sc.render(pto, pto.Scene(sd), params, flags=flags, with_sq=True)
        m = img[..., :3].astype(np.float64)
        return m, (sq / spp - m * m) * spp / (spp - 1), st

    (mb, vb, _), (mf, vf, sf) = mom(0), mom(sc.FLAGGED)
    z = float(np.max(np.abs((mf - mb).sum((0, 1))) / np.sqrt(((vf + vb) / spp).sum((0, 1)))))
    print("lamp 100 radii away: z", z, "variance ratio", vb.mean() / vf.mean())
    assert np.isfinite(mf).all() and sf.shadow_rays > 0 and mb.sum() > 0
    assert z < Z, z


def _wall_and_lamp(P, pto, r, flags, spp=256):
    """A wall lit by a lamp of radius r one unit in front of it, jitter off, max_depth 2, nothing else in the scene: (the checker's
    frame, the closed form, the smallest d / r). Every pixel's radiance is albedo * Le * (r^2 / d^2) * cos_s exactly — the
    cosine-weighted solid angle of a sphere above the horizon is pi sin^2(theta_max) cos(beta)."""
    import dataclasses
    import lens_checker as lc
    w = h = 16
    le, alb, eps = 1.0 / (r * r), 0.5, 1e-4
    c = np.array([0.013, 0.007, -1.0], np.float32)
    sd = lc.triangle_scene(P, w, h, [0, 0, -9, 0, 0, -9, 0, 0, -9], lc.camera(P, w, h, scale=0.05), emission=(0.0, 0.0, 0.0))
    mats = np.zeros(2, sd.mats.dtype)
    mats[0]["kind"], mats[0]["albedo"], mats[0]["ior"] = 0, (alb, alb, alb), 1.0
    mats[1]["kind"], mats[1]["emission"], mats[1]["ior"] = 0, (le, le, le), 1.0
    wall = np.array([[-2, -2, -2, 2, -2, -2, 2, 2, -2], [-2, -2, -2, 2, 2, -2, -2, 2, -2]], np.float32)
    sd = dataclasses.replace(sd, verts=wall, tri_mat=np.zeros(2, np.uint32), spheres=np.array([[*c, r]], np.float32), sph_mat=np.array([1], np.uint32),
                             mats=mats)
    params = P.make_params(w, h, spp=spp, max_depth=2, streams=1, ray_eps=eps)
    img, st, _ = sc.render(pto, pto.Scene(sd), params, flags=flags)
    assert st.n_sphere_lights == 1 and np.isfinite(img).all()
    ys, xs = np.mgrid[0:h, 0:w]
    cam = sd.cam
    sx, sy = (xs + 0.5) * cam.scale - cam.cx, (ys + 0.5) * cam.scale - cam.cy
    d = np.stack([sx, sy, -np.ones_like(sx)], -1).astype(np.float64)  # the camera at the origin looks down -z
    Pw = d * (2.0 / -d[..., 2:3]) + np.array([0.0, 0.0, eps])          # the wall z = -2, n = +z, lifted by ray_eps
    oc = c.astype(np.float64) - Pw
    d2 = (oc * oc).sum(-1)
    want = alb * float(np.float32(le)) * (float(np.float32(r)) ** 2 / d2) * (oc[..., 2] / np.sqrt(d2))
    return img[..., 0].astype(np.float64), want, float(np.sqrt(d2).min() / r)


@pytest.mark.parametrize("r", [1e-3, 1e-4])
def test_a_distant_lamp_has_its_closed_form(P, pto, r):
    """At 10^3 and at 10^4 radii (and more) the flagged checker holds to the closed form within 5e-4 per pixel: its float32 chain errs
    by 1e-6, its MIS weight differs from 1 by (pb / pl)^2 <= 1e-11, and cos_s varies over the cone by at most tan(beta) r / d <= 1.1e-3
    per sample, 3.4e-5 in the mean of 256. Measured: 4.5e-5 and 4.6e-6. (Brute force cannot serve here: it finds a lamp d / r away once
    in (d / r)^2 samples per vertex, and from some hundred radii on §4's sphere test, in which r^2 drops below an ulp of dot(oc, oc), sees
    the lamp as rounding noise.) Two mistakes miss the bound: 1.0f - cosm, which has 3 bits left at 10^3 radii and is 0 at 10^4
    (measured 0.17, and a black frame), and a shadow ray that its own lamp may block — that noise puts the lamp's surface radii early,
    inside tmax (measured: 0.63 and 1.0, a quarter and two thirds of the light lost)."""
    got, want, ratio = _wall_and_lamp(P, pto, r, sc.FLAGGED)
    naive, _, _ = _wall_and_lamp(P, pto, r, sc.FLAGGED | sc.NAIVE_OMC)
    blocked, _, _ = _wall_and_lamp(P, pto, r, sc.FLAGGED | sc.LAMP_BLOCKS)
    err = lambda a: float((np.abs(a - want) / want).max())
    print(r, "largest relative error", err(got), "naive", err(naive), "lamp blocks", err(blocked), 1 - blocked.sum() / want.sum())
    assert ratio >= 1e-3 / r * 1e3 and err(got) <= 5e-4, err(got)
    assert err(naive) > 5e-4 and err(blocked) > 5e-4
    assert r > 1e-4 or (naive == 0).all()


def test_product_does_not_reference_the_checker():
    for top in ("pathtracing_amd", "include", "host"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith((".py", ".cpp", ".h", ".hpp", ".hip", ".cs", "Makefile")):
                    txt = open(os.path.join(dirpath, f), errors="replace").read()
                    assert "sphere_light_ref" not in txt and "sphere_light_checker" not in txt and "sl_render" not in txt, f
