"""An independent physics pin for the part of docs/SPEC.md the reference cannot pin (it has no BSDFs and no path loop).

The HIP kernels and the C oracle are two transcriptions of one spec by one author; a misread formula would sit in both and every
HIP-vs-oracle test would stay green. These checks come from the other side: float64 numpy written from the physics (the GGX / Smith
BRDF evaluated directly and integrated by quadrature; a brute-force path tracer with numpy's own RNG, its own hemisphere
parametrisation and its own intersection code), sharing no sampling routine, RNG or weight formula with either implementation.
The oracle must agree within 3 sigma; a deliberately wrong masking term or a missing cosine makes the same checks fail.
CPU only: the oracle is the thing under test here (tests/test_gpu_parity.py then ties the HIP path to the oracle bit for bit).
"""
import ctypes as C

import numpy as np
import pytest

from numpy_radiance import numpy_radiance

# ---------------------------------------------------------------- (i) GGX rough metal: white-furnace directional albedo


def ggx_d(cos_h, a):
    return a * a / (np.pi * ((a * a - 1.0) * cos_h * cos_h + 1.0) ** 2)


def smith_g1(cos_v, a):
    return 2.0 * cos_v / (cos_v + np.sqrt(a * a + (1.0 - a * a) * cos_v * cos_v))


def wrong_g1(cos_v, a):  # Schlick's k = a/2 approximation: close, but not what the spec says
    k = a / 2.0
    return cos_v / (cos_v * (1.0 - k) + k)


def directional_albedo(cos_o, a, g1=smith_g1, n_theta=1500, n_phi=3000):
    """Integral over the hemisphere of f(wo, wi) cos_i with f = D(h) G1(wo) G1(wi) / (4 cos_o cos_i), F = 1 (white furnace),
    by midpoint quadrature in (theta_i, phi_i). Pure BRDF evaluation: no sampling routine involved."""
    th = (np.arange(n_theta) + 0.5) * (np.pi / 2) / n_theta
    ph = (np.arange(n_phi) + 0.5) * (2 * np.pi) / n_phi
    st, ct = np.sin(th)[:, None], np.cos(th)[:, None]
    wi = np.stack([st * np.cos(ph)[None, :], st * np.sin(ph)[None, :], np.broadcast_to(ct, (n_theta, n_phi))], -1)
    wo = np.array([np.sqrt(1.0 - cos_o * cos_o), 0.0, cos_o])
    h = wi + wo
    h /= np.linalg.norm(h, axis=-1, keepdims=True)
    integrand = ggx_d(h[..., 2], a) * g1(cos_o, a) * g1(wi[..., 2], a) / (4.0 * cos_o)  # = f * cos_i
    return float((integrand * st).sum() * (np.pi / 2 / n_theta) * (2 * np.pi / n_phi))


def oracle_metal_weights(pto, cos_o, a, n, rng):
    """Mean and standard error of the oracle's sampled weight W (albedo 1 => W = its masking term), failed samples counted as 0."""
    m = np.zeros(1, pto.MATERIAL_DTYPE)
    m["kind"], m["albedo"], m["roughness"], m["ior"] = pto.lib.PTO_METAL if hasattr(pto.lib, "PTO_METAL") else 1, 1.0, a, 1.5
    d = (C.c_float * 3)(-float(np.sqrt(1 - cos_o * cos_o)), 0.0, -float(cos_o))  # incoming direction: wo = -d
    nrm = (C.c_float * 3)(0.0, 0.0, 1.0)
    wi, W, side = (C.c_float * 3)(), (C.c_float * 3)(), C.c_float()
    u = rng.random((n, 2))
    w = np.zeros(n)
    below = 0
    for i in range(n):
        if pto.lib.pto_bsdf_sample(m.ctypes.data_as(C.c_void_p), d, nrm, 1, float(u[i, 0]), float(u[i, 1]), 0.5, wi, W, C.byref(side)):
            w[i] = W[0]
            below += wi[2] <= 0.0
    assert below == 0  # an accepted direction is above the surface
    return w.mean(), w.std(ddof=1) / np.sqrt(n)


@pytest.mark.parametrize("alpha", [0.2, 0.5, 0.8])
def test_ggx_metal_white_furnace_albedo(pto, alpha):
    rng = np.random.default_rng(1234)
    for cos_o in (0.9, 0.5, 0.25):
        want = directional_albedo(cos_o, alpha)
        got, se = oracle_metal_weights(pto, cos_o, alpha, 60000, rng)
        assert abs(got - want) <= 3.0 * se + 2e-4, (alpha, cos_o, got, want, se)  # 2e-4: quadrature + float32 in the oracle
        assert 0.0 < want <= 1.0 + 1e-9  # single scattering never creates energy


def test_a_wrong_masking_term_would_be_caught(pto):
    """Sensitivity of the check above: with Schlick's k = alpha/2 in place of the Smith G1 of the spec the quadrature moves by far
    more than the 3 sigma the oracle is held to."""
    rng = np.random.default_rng(99)
    alpha, cos_o = 0.5, 0.5
    got, se = oracle_metal_weights(pto, cos_o, alpha, 60000, rng)
    right, wrong = directional_albedo(cos_o, alpha), directional_albedo(cos_o, alpha, g1=wrong_g1)
    assert abs(got - right) <= 3.0 * se + 2e-4
    assert abs(got - wrong) > 10.0 * se


# ---------------------------------------------------------------- (ii) converged Cornell pixels against a brute-force float64 tracer


def test_converged_cornell_pixels_match_an_independent_estimator(P, pto):
    """16 pixels (a 4 x 4 frame, so every pixel averages a sixteenth of the view) of the Cornell box at 16384 spp from the oracle
    against 30000 brute-force float64 paths per pixel: every channel within 3 combined sigma (a few would be allowed to stray by
    chance: at most 2 of 48 beyond 3 sigma, none beyond 5)."""
    w = h = 4
    sd = P.make_scene(P.native.PT_SCENE_CORNELL, 0, 0x5EED0001, w, h)
    spp = 16384
    ref, _ = pto.render(pto.Scene(sd), P.make_params(w, h, spp=spp, max_depth=8, rr_start=3, seed=77))
    rng = np.random.default_rng(2026)
    mean, err = numpy_radiance(sd, w, h, 30000, 8, 3, rng)
    sigma = np.sqrt(err ** 2 + (err * np.sqrt(30000 / spp)) ** 2)  # the oracle's own noise, from the same per-path spread
    z = np.abs(ref[..., :3] - mean) / np.maximum(sigma, 1e-6)
    assert (z > 3.0).sum() <= 2 and z.max() < 5.0, (z.max(), (z > 3).sum())
    assert (z * z).sum() < 48 + 5 * np.sqrt(2 * 48), (z * z).sum()  # chi-square over the 48 channel values: 48 +- 9.8 expected
    assert ref[..., :3].mean() > 0.05  # the light is seen: not a frame of zeros agreeing with zeros


def test_a_missing_cosine_would_be_caught(P, pto):
    """The same comparison with a deliberately wrong estimator (uniform hemisphere sampling used as if it were cosine-weighted)
    lands far outside the band."""
    w = h = 4
    sd = P.make_scene(P.native.PT_SCENE_CORNELL, 0, 0x5EED0001, w, h)
    ref, _ = pto.render(pto.Scene(sd), P.make_params(w, h, spp=4096, max_depth=8, rr_start=3, seed=5))
    mean, err = numpy_radiance(sd, w, h, 16000, 8, 3, np.random.default_rng(1), drop_cosine=True)
    z = np.abs(ref[..., :3] - mean) / np.maximum(err * np.sqrt(1.0 + 16000 / 4096), 1e-6)
    assert (z * z).sum() > 48 + 15 * np.sqrt(2 * 48), (z * z).sum()  # chi-square: far outside what 48 honest values give


def test_converged_glass_and_metal_pixels_match_an_independent_estimator(P, pto):
    """BASELINE config C4's scene (Cornell + glass sphere, rough gold, mirror, Lambert) at max depth 16: the oracle's converged 4 x 4
    frame against the float64 tracer that samples the GGX lobe by D(h) cos(theta_h) instead of visible normals, picks glass lobes
    from its own Snell / Fresnel code and plays a different Russian roulette. Caustic paths make the per-pixel spread heavy-tailed,
    hence the wider band than for the Lambert box: no channel beyond 5 combined sigma, at most 3 of 48 beyond 3."""
    w = h = 4
    sd = P.make_scene(P.native.PT_SCENE_CORNELL_GLASS, 0, 0x5EED0001, w, h)
    spp, n = 32768, 40000
    ref, _ = pto.render(pto.Scene(sd), P.make_params(w, h, spp=spp, max_depth=16, rr_start=3, seed=4242))
    mean, err = numpy_radiance(sd, w, h, n, 16, 3, np.random.default_rng(7), own_roulette=True)
    sigma = np.sqrt(err ** 2 + (err * np.sqrt(n / spp)) ** 2)
    z = np.abs(ref[..., :3] - mean) / np.maximum(sigma, 1e-6)
    assert (z > 3.0).sum() <= 3 and z.max() < 5.0, (z.max(), (z > 3).sum())
    assert (z * z).sum() < 48 + 6 * np.sqrt(2 * 48), (z * z).sum()


def aim(sd, target, half_width):
    """Point the scene's pinhole camera at `target` with a field of view of +-half_width (tangent) across the frame height."""
    cam = sd.cam
    o = np.array(cam.origin[:], np.float64)
    f = np.asarray(target, np.float64) - o
    f /= np.linalg.norm(f)
    r = np.cross(f, [0.0, 1.0, 0.0]); r /= np.linalg.norm(r)
    u = np.cross(r, f)
    for k in range(3):
        cam.forward[k] = f[k]; cam.right[k] = r[k] * half_width; cam.up[k] = -u[k] * half_width  # image row 0 is the top


@pytest.mark.parametrize("what,target,half_width,wrong", [("glass sphere", (-0.45, -0.65, 0.25), 0.11, "no_reflection"),
                                                         ("rough gold sphere", (0.5, -0.65, -0.3), 0.09, "no_masking")])
def test_close_ups_of_the_specular_spheres(P, pto, what, target, half_width, wrong):
    """The same comparison with the camera zoomed onto C4's glass sphere and onto its rough-metal sphere, so that those BSDFs fill
    the 16 pixels: the honest independent estimator agrees with the oracle; one that never reflects at the glass surface /
    leaves out the Smith masking term (gold roughened to alpha 0.6 for this close-up) does not."""
    w = h = 4
    sd = P.make_scene(P.native.PT_SCENE_CORNELL_GLASS, 0, 0x5EED0001, w, h)
    aim(sd, target, half_width)
    if wrong == "no_masking":
        sd.mats["roughness"][sd.mats["kind"] == 1] *= 4.0  # gold at alpha 0.6 (the mirror stays 0): where the Smith terms matter
    spp, n = 16384, 24000
    ref, _ = pto.render(pto.Scene(sd), P.make_params(w, h, spp=spp, max_depth=16, rr_start=3, seed=99))
    for bad in (None, wrong):
        mean, err = numpy_radiance(sd, w, h, n, 16, 3, np.random.default_rng(3), own_roulette=True, wrong=bad)
        sigma = np.sqrt(err ** 2 + (err * np.sqrt(n / spp)) ** 2)
        z = np.abs(ref[..., :3] - mean) / np.maximum(sigma, 1e-6)
        chi2 = (z * z).sum()
        if bad is None:
            assert (z > 3.0).sum() <= 3 and z.max() < 5.0 and chi2 < 48 + 6 * np.sqrt(2 * 48), (what, z.max(), (z > 3).sum(), chi2)
        else:
            assert chi2 > 48 + 15 * np.sqrt(2 * 48), (what, bad, chi2)
