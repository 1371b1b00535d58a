"""pt_denoise (docs/SPEC.md §8) against float64, without a GPU: the scalar checker of tests/denoise_ref/ pass by pass against
tests/denoise64.py's exact pass and its derived per-pass bound, on random and adversarial synthetic fields over the whole accepted parameter
domain; every accepted parameter set gives a finite image; the checker's guides against the float64 caster; and negative controls, wrong
variants of a pass that the comparison must reject by a wide margin.

tests/test_gpu_denoise64.py holds the device to the same reference."""
import numpy as np
import pytest

import adversarial_scenes as adv
import denoise64 as d64
import denoise_checker as dc

FLT_MAX = d64.FLT_MAX
MISS_F = np.array([dc.MISS], np.uint32).view(np.float32)[0]
# each σ over a log grid: a subnormal, the smallest normal, 2^±60, ordinary values, one that is not a power of two, FLT_MAX
SIGMA_GRID = [2.0 ** -140, 2.0 ** -126, 2.0 ** -60, 2.0 ** -8, 0.3, 1.0, 2.0 ** 8, 3e19, 2.0 ** 60, FLT_MAX]
SIGMAS = ("sigma_color", "sigma_normal", "sigma_depth", "sigma_albedo")
# every colour component below this magnitude gives a finite image (SPEC §8.2)
COLOUR_LIMIT = 2.0 ** 126


def field(kind, h, w, seed=0):
    """(image, guides) of a synthetic (h, w) frame: `kind` picks the colours and guides."""
    rng = np.random.default_rng(seed)
    img = np.zeros((h, w, 4), np.float32)
    img[..., 3] = rng.uniform(0, 1, (h, w))
    n = rng.normal(size=(h, w, 3)).astype(np.float32)
    n = n / np.sqrt((n * n).sum(-1, keepdims=True), dtype=np.float32)  # unit in float64 terms, not exactly in f32
    g = np.zeros((h, w, 8), np.float32)
    g[..., 0:3] = n
    g[..., 3] = rng.uniform(1, 3, (h, w))
    g[..., 4:7] = rng.uniform(0, 1, (h, w, 3))
    g[..., 7] = rng.integers(0, 6, (h, w)).astype(np.uint32).view(np.float32)
    miss = rng.uniform(size=(h, w)) < 0.2
    if kind == "ldr":
        img[..., :3] = rng.uniform(0, 1, (h, w, 3))
    elif kind == "hdr":  # log-uniform up to 2^100, fireflies, some exact zeros and negatives
        img[..., :3] = 2.0 ** rng.uniform(-30, 100, (h, w, 3)) * rng.uniform(0.5, 1, (h, w, 3))
        img[rng.uniform(size=(h, w)) < 0.02, :3] *= 2.0 ** 20
        img[rng.uniform(size=(h, w)) < 0.1, :3] = 0.0
        img[rng.uniform(size=(h, w)) < 0.05, :3] *= -1.0
    elif kind == "firefly":  # a dim image with a few very bright pixels
        img[..., :3] = rng.uniform(0, 0.1, (h, w, 3))
        img[rng.uniform(size=(h, w)) < 0.01, :3] = 1e6
    elif kind == "const":
        img[..., :3] = 0.7
        img[: h // 2, :, :3] = 0.0
    elif kind == "zeros":
        pass
    elif kind == "depth":  # t from 2^-100 to 2^100, normals off unit length by up to 2^-20
        img[..., :3] = rng.uniform(0, 4, (h, w, 3))
        g[..., 3] = 2.0 ** rng.uniform(-100, 100, (h, w))
        g[..., 0:3] *= (1 + rng.uniform(-2.0 ** -20, 2.0 ** -20, (h, w, 1))).astype(np.float32)
    elif kind == "smooth":  # a smooth surface: taps with small x where the weight error matters most
        yy, xx = np.mgrid[0:h, 0:w] / max(h, w)
        img[..., 0], img[..., 1], img[..., 2] = 0.5 + 0.3 * np.sin(5 * xx), 0.4 + 0.2 * yy, 0.3
        img[..., :3] += rng.normal(0, 0.05, (h, w, 3)).astype(np.float32)
        nn = np.stack([0.1 * xx, 0.1 * yy, np.ones_like(xx)], -1)
        g[..., 0:3] = (nn / np.linalg.norm(nn, axis=-1, keepdims=True)).astype(np.float32)
        g[..., 3] = 2 + xx + 0.5 * yy
        g[..., 4:7] = 0.5 + 0.01 * rng.normal(size=(h, w, 3))
        g[..., 7] = np.zeros((h, w), np.uint32).view(np.float32)
        miss[:] = False
        miss[:, : w // 8] = True
    else:
        raise ValueError(kind)
    g[miss, 0:3], g[miss, 3], g[miss, 4:7], g[miss, 7] = 0.0, np.inf, 0.0, MISS_F
    return img, g


KINDS = ["ldr", "hdr", "firefly", "const", "zeros", "depth", "smooth"]


def passes(img, g, p, prm, n):
    """Run the checker pass by pass and compare each pass with the float64 pass of the checker's own input. Returns the worst ratio."""
    cur, worst = img, 0.0
    for i in range(n):
        out = dc.one_pass(cur, g, i, p)
        r, at = d64.pass_error(out, cur, g, i, prm)
        assert r <= 1.0, (i, r, at)
        worst = max(worst, r)
        cur = out
    return worst


def check_params(img, g, n=None, **kw):
    p = dc.params(**kw)
    prm = d64.resolve64(**kw)
    n = n if n is not None else prm["iterations"]
    worst = passes(img, g, p, prm, n)
    if n == prm["iterations"]:  # and the pass-by-pass chain is dr_filter's
        cur = img
        for i in range(n):
            cur = dc.one_pass(cur, g, i, p)
        assert np.array_equal(dc.filter(img, g, p).view(np.uint32), cur.view(np.uint32))
    return worst


@pytest.mark.parametrize("kind", KINDS)
def test_synthetic_fields_pass_by_pass(kind):
    img, g = field(kind, 37, 29, seed=KINDS.index(kind))
    for flags in (0, dc.NO_EDGE_STOPS):
        check_params(img, g, iterations=8, flags=flags)


def test_default_resolution_matches_the_spec():
    assert d64.resolve64() == dict(iterations=4, sigma_color=16.0, sigma_normal=0.0625, sigma_depth=0.0078125, sigma_albedo=0.25, edge=True)
    assert tuple(dc.defaults()) == (4, 16.0, 0.0625, 0.0078125, 0.25)
    for bad in (dict(iterations=9), dict(flags=4), dict(sigma_color=-1.0), dict(sigma_depth=float("inf")), dict(sigma_normal=float("nan"))):
        assert d64.resolve64(**bad) is None
    assert d64.resolve64(sigma_albedo=FLT_MAX)["sigma_albedo"] == FLT_MAX


@pytest.mark.parametrize("which", SIGMAS)
def test_finite_over_the_sigma_grid(which):
    """Each σ over its log grid, the others at their defaults, 8 passes: every pass is finite and within the float64 bound."""
    for kind in ("ldr", "hdr", "depth"):
        img, g = field(kind, 19, 23, seed=5)
        for v in SIGMA_GRID:
            check_params(img, g, iterations=8, **{which: v})


def test_finite_at_the_corners_of_the_issue():
    """The parameter sets that gave NaN for every pixel: an overflowing inverse scale times a zero difference, an overflowed colour
    difference times a vanished scale, and a centre tap that lost its weight to x_n. Each is accepted by pt_denoise; each must give a
    finite image that the float64 pass bounds."""
    rng = np.random.default_rng(11)
    h = w = 16
    n = rng.normal(size=(h, w, 3)).astype(np.float32)
    n = n / np.sqrt((n * n).sum(-1, keepdims=True), dtype=np.float32)
    g = np.zeros((h, w, 8), np.float32)
    g[..., 0:3], g[..., 3], g[..., 4:7] = n, rng.uniform(1, 3, (h, w)), 0.5
    img = np.full((h, w, 4), 0.5, np.float32)
    cases = [(img, g, dict(iterations=1, sigma_color=2e-20)),
             (img, g, dict(iterations=8, sigma_color=1e-18)),
             (img, g, dict(sigma_normal=2.0 ** -126)),
             (img, g, dict(sigma_albedo=2e-20))]
    tiny = g.copy()
    tiny[..., 3] = rng.uniform(1, 3, (h, w)) * 1e-9
    cases.append((img, tiny, dict(sigma_depth=1e-30)))
    tiny = g.copy()
    tiny[..., 3] = 1e-37
    cases.append((img, tiny, dict()))
    hdr = img.copy()
    hdr[..., :3] = rng.uniform(0, 1, (h, w, 3)) * 1e20
    cases.append((hdr, g, dict(sigma_color=1e30)))
    for k, (im, gg, kw) in enumerate(cases):
        out = dc.filter(im, gg, dc.params(**kw))
        assert np.isfinite(out).all(), (k, kw, int((~np.isfinite(out)).any(axis=2).sum()))
        check_params(im, gg, **kw)


def test_finite_at_the_colour_limit():
    """Colours up to the stated limit, positive and negative, with every σ at its extremes: finite, and within the bound."""
    rng = np.random.default_rng(12)
    img, g = field("ldr", 11, 13, seed=12)
    img[..., :3] = (COLOUR_LIMIT * rng.choice([-1.0, -0.5, 0.0, 0.5, 1.0], (11, 13, 3))).astype(np.float32)
    for v in (2.0 ** -149, 2.0 ** -126, 1.0, FLT_MAX):
        check_params(img, g, iterations=8, sigma_color=v, sigma_normal=v, sigma_depth=v, sigma_albedo=v)


@pytest.mark.parametrize("h,w", [(1, 1), (1, 17), (17, 1), (3, 2), (5, 70)])
def test_sizes_and_steps_beyond_the_image(h, w):
    """1x1, 1xN, Nx1 and frames smaller than the step of the later passes (every tap but the centre is outside)."""
    for kind in ("ldr", "hdr", "smooth"):
        img, g = field(kind, h, w, seed=h * 100 + w)
        check_params(img, g, iterations=8)
        check_params(img, g, iterations=8, sigma_color=0.3, sigma_normal=0.7, sigma_depth=3.0, sigma_albedo=0.05)


def test_finite_when_every_tap_loses_its_weight():
    """Huge colour differences and a tiny σ_c give every neighbour weight 0. Where the f32 |n|² is below 1 and σ_n is tiny, the centre
    tap's x_n = max(0, 1 - |n|²)·in overflows D as well, so sw = 0: the pixel is kept (SPEC §8.2). Elsewhere the centre tap alone
    weighs h_2² and (c·h_2²)·(1/h_2²) rounds twice: 2 ulp. Either way the pixel comes back."""
    img, g = field("ldr", 9, 9, seed=3)
    img[..., :3] = np.arange(81 * 3, dtype=np.float32).reshape(9, 9, 3) * 1e6
    out = dc.filter(img, g, dc.params(1, sigma_color=2.0 ** -100, sigma_normal=2.0 ** -100))
    assert np.isfinite(out).all() and np.array_equal(out[..., 3], img[..., 3])
    assert (np.abs(out[..., :3] - img[..., :3]) <= 2 * np.spacing(img[..., :3])).all()


def test_guides_of_generator_and_adversarial_scenes(P, pto):
    """The checker's guides against guides64: ids agree except in the classes the caster cannot settle, normal and t within the
    derived bound on agreeing hits, albedo exact, misses exact."""
    N = P.native
    w, h = 48, 32
    scenes = {"cornell": P.make_scene(N.PT_SCENE_CORNELL, 0, 3, w, h), "glass": P.make_scene(N.PT_SCENE_CORNELL_GLASS, 0, 3, w, h),
              "tess": P.make_scene(N.PT_SCENE_CORNELL_TESS, 3000, 3, w, h), "layers": adv.stacked_layers(w, h),
              "duplicates": adv.duplicates(w, h)[0], "spheres64": adv.sphere_list(64, w, h),
              "inside_sphere": adv.sphere_list(8, w, h, camera_inside=True)}
    scenes["axis"] = adv.axis_camera(scenes["cornell"], 49, 33)
    scenes["floor"] = adv.floor_camera(scenes["cornell"], 49, 33)
    for k in (-30, 30):
        scenes[f"cornell_2^{k}"] = adv.scaled(scenes["glass"], k)
    for name, sd in scenes.items():
        ww, hh = (49, 33) if name in ("axis", "floor") else (w, h)
        g = d64.guides64(pto, sd, ww, hh)
        agree, rn, rt = d64.compare_guides(dc.guides(pto, pto.Scene(sd), ww, hh), g, ww, hh)
        assert agree >= 0.95 * ww * hh, (name, agree)


# ------------------------------------------------------------------------------------------------------------------ negative controls
NEGATIVE = {dc.SIGMA_C_FIXED: ("smooth", 2), dc.XZ_NO_STEP: ("smooth", 2), dc.D_LINEAR: ("smooth", 0), dc.WRONG_TAP: ("ldr", 0),
            dc.NO_MISS_SKIP: ("ldr", 0)}


@pytest.mark.parametrize("variant", sorted(NEGATIVE))
def test_negative_controls(variant):
    """A wrong pass (σ_c not halved per pass, x_z without 1/s, D(x) = 1 + x, one wrong B3 tap, the miss/hit skip dropped) fails the
    float64 comparison by a wide margin, on an input where the right pass passes it."""
    kind, i = NEGATIVE[variant]
    img, g = field(kind, 40, 48, seed=21)
    prm = d64.resolve64(sigma_color=0.25, sigma_depth=0.05)
    p = dc.params(sigma_color=0.25, sigma_depth=0.05)
    assert d64.pass_error(dc.one_pass(img, g, i, p), img, g, i, prm)[0] <= 1.0
    bad = dc.one_pass(img, g, i, p, variant=variant)
    r, _ = d64.pass_error(bad, img, g, i, prm)
    assert r > 100.0, (variant, r)
