"""Environment-map lighting (docs/SPEC.md §11) without a GPU: the octahedral map, the sampling table the product builds on a detached
scene against the scalar checker of tests/env_ref/ bit for bit, the argument checks, and the checker itself — against the oracle where
the environment is constant or black, and against its own plain estimator where the map is sampled with MIS.

The device is held to the checker bit for bit by tests/test_gpu_env.py."""
import ctypes as C
import os

import numpy as np
import pytest

import env_checker as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 32       # image side
SPP = 2048   # samples per pixel of the statistical tests
Z = 4.0      # the statistical tests' bound, in standard deviations
SOUP = 20000  # triangles of the statistical tests' soup: C3's triangles are small, 500 of them cover 0.2 % of this camera's pixels


# ---------------------------------------------------------------------------------------------------------------------------- the map
@pytest.mark.parametrize("n", [1, 2, 5, 8, 64])
def test_texel_centres_round_trip(n):
    for j in range(n):
        for i in range(n):
            d = ec.decode(np.float32(-1.0 + (2 * i + 1) / n), np.float32(-1.0 + (2 * j + 1) / n))
            assert abs(float(np.linalg.norm(d.astype(np.float64))) - 1.0) < 1e-6
            gi, gj, s = ec.encode(d, n)
            assert (gi, gj) == (i, j), (n, i, j)
            assert abs(s - float(np.abs(d.astype(np.float64)).sum())) < 1e-6


def test_axes_and_fold_lines():
    """Where §11 puts the six axes and the directions on the fold lines, on an 8 x 8 map: u = v = 0 is +z, the corners are -z, and
    sgn(+0) = +1, sgn(-0) = -1 decide the side of the lower half's folds."""
    n = 8
    assert ec.encode((0, 0, 1), n)[:2] == (4, 4)       # u = v = 0 -> floor(0.5 * 8)
    assert ec.encode((1, 0, 0), n)[:2] == (7, 4)       # u = 1 clamps to the last column
    assert ec.encode((-1, 0, 0), n)[:2] == (0, 4)
    assert ec.encode((0, 1, 0), n)[:2] == (4, 7)
    assert ec.encode((0, -1, 0), n)[:2] == (4, 0)
    assert ec.encode((0.0, 0.0, -1.0), n)[:2] == (7, 7)    # px = py = +0: (1 - 0) * sgn(+0) = +1 both
    assert ec.encode((-0.0, 0.0, -1.0), n)[:2] == (0, 7)   # px = -0: u = -1
    assert ec.encode((0.0, -0.0, -1.0), n)[:2] == (7, 0)
    assert ec.encode((-0.0, -0.0, -1.0), n)[:2] == (0, 0)
    h = np.float32(np.sqrt(0.5))
    assert ec.encode((h, 0.0, -0.0), n)[:2] == (7, 4)      # d.z = -0.0 is not < 0: the upper half's formula, (u, v) = (1, 0)
    assert ec.encode((h, 0.0, -h), n)[:2] == (7, 6)        # lower half, py = +0: u = (1 - 0) * 1, v = (1 - 0.5) * sgn(+0) = 0.5 -> row floor(0.75 * 8)
    assert ec.encode((h, -0.0, -h), n)[:2] == (7, 2)       # py = -0: v = -0.5 -> row floor(0.25 * 8)
    # the four corners decode to -z, the centre to +z, the edge midpoints to the +-x / +-y axes
    for u, v in ((1, 1), (-1, 1), (1, -1), (-1, -1)):
        assert np.array_equal(ec.decode(u, v), np.array([0, 0, -1], np.float32))
    assert np.array_equal(ec.decode(0, 0), np.array([0, 0, 1], np.float32))
    assert np.array_equal(ec.decode(1, 0), np.array([1, 0, 0], np.float32))
    assert np.array_equal(ec.decode(0, -1), np.array([0, -1, 0], np.float32))


@pytest.mark.parametrize("n", [1, 2, 5, 8, 64])
def test_texel_solid_angles_sum_to_4pi(n):
    """The table weighs texel k by sc^3 * dA (sc at the texel centre): a midpoint rule for d omega = s^3 dA, which converges as
    1 / n^2 (n = 64: 1e-4 relative); a 512^2 midpoint sum is 4 pi to 1e-6."""
    total = sum(ec.texel_solid_angle(i, j, n) for j in range(n) for i in range(n))
    assert abs(total / (4 * np.pi) - 1.0) < {1: 0.7, 2: 0.1, 5: 0.02, 8: 0.01, 64: 2e-4}[n]
    t = (np.arange(512) + 0.5) / 256.0 - 1.0
    u, v = np.meshgrid(t, t)
    z = 1.0 - np.abs(u) - np.abs(v)
    x = np.where(z < 0, (1 - np.abs(v)) * np.sign(u), u)
    y = np.where(z < 0, (1 - np.abs(u)) * np.sign(v), v)
    s = 1.0 / np.sqrt(x * x + y * y + z * z)  # the 1-norm of the unit direction: the octahedron point has 1-norm 1
    fine = (s ** 3).sum() * (2.0 / 512) ** 2
    assert abs(fine / (4 * np.pi) - 1.0) < 1e-5
    if n == 64:
        assert abs(ec.texel_solid_angle(31, 40, 64) / ((np.abs(ec.decode(np.float32(-1 + 63 / 64), np.float32(-1 + 81 / 64)).astype(np.float64)).sum() ** 3) * (2 / 64) ** 2) - 1) < 1e-6


# -------------------------------------------------------------------------------------------------------------------------- the table
def maps():
    rng = np.random.default_rng(7)
    hot = np.zeros((8, 8, 3), np.float32)
    hot[5, 2] = (1000.0, 10.0, 0.5)
    rows = rng.random((8, 8, 3), dtype=np.float32)
    rows[0] = 0
    rows[3] = 0
    rows[7] = 0
    return {
        "constant": np.full((8, 8, 3), 0.75, np.float32),
        "hot": hot,
        "random": (rng.random((64, 64, 3), dtype=np.float32) * 10).astype(np.float32),
        "n1": np.array([[[0.2, 0.5, 3.0]]], np.float32),
        "n5": rng.random((5, 5, 3), dtype=np.float32),
        "zero_rows": rows,
        "black": np.zeros((4, 4, 3), np.float32),
    }


class Detached:
    """A context-less pt_scene: host table only."""

    def __init__(self, P):
        self.N = P.native
        self.s = C.c_void_p()
        assert self.N.lib.pt_scene_create(None, C.byref(self.s)) == 0

    def set(self, rgb, n=None):
        a = None if rgb is None else np.ascontiguousarray(rgb, np.float32)
        return self.N.lib.pt_scene_set_environment(self.s, None if a is None else a.ctypes.data, (0 if a is None else a.shape[0]) if n is None else n)

    def info(self):
        i = self.N.pt_environment_info()
        assert self.N.lib.pt_scene_environment_info(self.s, C.byref(i)) == 0
        return i

    def read(self):
        n = self.info().n
        tex, mcdf, ccdf = np.zeros((n, n, 4), np.float32), np.zeros(n, np.float32), np.zeros((n, n), np.float32)
        st = self.N.lib.pt_scene_environment_read(self.s, tex.ctypes.data, mcdf.ctypes.data, ccdf.ctypes.data, n * n)
        return st, tex, mcdf, ccdf

    def close(self):
        self.N.lib.pt_scene_destroy(self.s)


@pytest.fixture()
def detached(P):
    d = Detached(P)
    yield d
    d.close()


@pytest.mark.parametrize("name", ["constant", "hot", "random", "n1", "n5", "zero_rows", "black"])
def test_table_is_the_checkers(P, detached, name):
    """pt_scene_environment_read on a detached scene = the checker's table, bit for bit; and the table's own invariants."""
    rgb = maps()[name]
    n = rgb.shape[0]
    assert detached.set(rgb) == 0
    st, tex, mcdf, ccdf = detached.read()
    info = detached.info()
    want_tex, want_m, want_c, lit, total = ec.table(rgb)
    assert st == 0 and info.n == n and info.lit == lit and info.total == total and info.device_bytes == 0
    for got, want in ((tex, want_tex), (mcdf, want_m), (ccdf, want_c)):
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
    assert np.array_equal(tex[..., :3], rgb) and mcdf[-1] == 1.0 and (ccdf[:, -1] == 1.0).all()
    assert (np.diff(mcdf) >= 0).all() and (np.diff(ccdf, axis=1) >= 0).all()
    if name == "black":
        assert lit == 0 and (tex[..., 3] == 0).all() and (mcdf == 1).all() and (ccdf == 1).all()
    else:
        assert lit == 1
        # p is a density over the map's square [-1, 1]^2, of area 4: its mean over the texels is 1 / 4
        assert abs(float(tex[..., 3].astype(np.float64).mean()) * 4.0 - 1.0) < 1e-6
    if name == "zero_rows":
        assert (ccdf[[0, 3, 7]] == 1).all() and mcdf[0] == 0 and mcdf[3] == mcdf[2] and (tex[[0, 3, 7], :, 3] == 0).all()
    if name == "hot":
        assert tex[5, 2, 3] == 16.0 and mcdf[4] == 0 and mcdf[5] == 1 and ccdf[5, 1] == 0 and ccdf[5, 2] == 1


def test_argument_checks_and_removal(P, detached):
    N = P.native
    bad = N.PT_ERR_INVALID_ARGUMENT
    assert detached.info().n == 0
    assert detached.read()[0] == bad                                   # nothing set
    good = maps()["n5"]
    assert detached.set(good) == 0
    before = detached.read()
    refused = [
        (None, 4),                                                     # NULL with n > 0
        (good, 0),                                                     # an array with n == 0
        (np.zeros((2049, 1, 3), np.float32), 2049),                    # n too large (refused before the array is read)
    ]
    for k, v in ((0, -1.0), (7, np.nan), (74, np.inf), (3, -np.inf)):
        m = good.copy()
        m.reshape(-1)[k] = v
        refused.append((m, None))
    neg_zero = good.copy()
    neg_zero[0, 0, 0] = -0.0                                           # -0.0 >= 0: accepted
    for rgb, n in refused:
        assert detached.set(rgb, n) == bad
        after = detached.read()
        assert after[0] == 0 and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(after[1:], before[1:]))
    assert b"pt_scene_set_environment" in N.lib.pt_last_error(None)
    assert N.lib.pt_scene_set_environment(None, None, 0) == bad
    assert N.lib.pt_scene_environment_info(detached.s, None) == bad
    tex, mcdf, ccdf = before[1:]
    assert N.lib.pt_scene_environment_read(detached.s, tex.ctypes.data, mcdf.ctypes.data, ccdf.ctypes.data, 24) == bad  # room for 24 < 25 texels
    assert detached.set(neg_zero) == 0 and detached.info().lit == 1
    assert detached.set(np.zeros((2048, 2048, 3), np.float32)) == 0 and detached.info().n == 2048 and detached.info().lit == 0
    assert detached.set(None) == 0 and detached.info().n == 0 and detached.info().lit == 0 and detached.info().total == 0
    assert detached.read()[0] == bad
    assert detached.set(None) == 0                                     # removing nothing is fine


def test_host_helpers(P):
    """sun_sky_environment is deterministic and puts its sun where it says; environment_from_latlong of a constant image is constant
    and keeps a bright +y pole cap at +y."""
    a, b = ec.sun_sky(P), ec.sun_sky(P)
    assert a.dtype == np.float32 and a.shape == (64, 64, 3) and np.array_equal(a, b) and np.isfinite(a).all() and (a >= 0).all()
    d = np.asarray(ec.SUN_DIR) / np.linalg.norm(ec.SUN_DIR)
    i, j, _ = ec.encode(d.astype(np.float32), 64)
    assert np.allclose(a[j, i], (40.3, 36.4, 30.6)) and np.allclose(a.min((0, 1)), (0.3, 0.4, 0.6))
    assert np.allclose(P.environment_from_latlong(np.full((16, 32, 3), 0.5), 8), 0.5)
    img = np.zeros((64, 128, 3))
    img[:4] = 9.0  # the cap within 11 degrees of +y
    m = P.environment_from_latlong(img, 16)
    i, j, _ = ec.encode((0, 1, 0), 16)
    assert m[j, i].min() > 0 and m[0, 8].max() == 0 and m.shape == (16, 16, 3) and m.dtype == np.float32


# ------------------------------------------------------------------------------------------------------------------------- the checker
def test_constant_environment_is_the_sky(P, pto):
    """The checker's plain frame under a constant environment c = pto_render with sky = c, bit for bit, with the same rays."""
    import dataclasses
    c = (0.7, 0.9, 1.3)
    params = P.make_params(S, S, spp=16, max_depth=8, streams=4)
    for name in ("soup", "cornell", "glass"):
        sd = dataclasses.replace(ec.scene(P, name, S, S, 2000), sky=np.asarray(c, np.float32))
        ref, ost = pto.render(pto.Scene(sd), params)
        for n in (1, 5, 64):
            img, st, _ = ec.render(pto, pto.Scene(sd), params, env=np.full((n, n, 3), c, np.float32))
            assert np.array_equal(img, ref) and st.ext_rays == ost.rays and st.shadow_rays == 0, (name, n)
        none, st, _ = ec.render(pto, pto.Scene(sd), params)  # no environment: the scene's sky
        assert np.array_equal(none, ref)


def test_black_environment_is_a_black_sky(P, pto):
    """An all-black environment (lit = 0) = sky 0, plain and with NEE (where the triangle lights keep psel = 1: tests/nee_ref's frame)."""
    import dataclasses
    import nee_checker as nc
    params = P.make_params(S, S, spp=16, max_depth=8, streams=4)
    for name in ("soup", "cornell"):
        sd = dataclasses.replace(ec.scene(P, name, S, S, 2000), sky=np.zeros(3, np.float32))
        black = np.zeros((4, 4, 3), np.float32)
        ref, ost = pto.render(pto.Scene(sd), params)
        img, st, _ = ec.render(pto, pto.Scene(sd), params, env=black)
        assert np.array_equal(img, ref) and st.ext_rays == ost.rays and st.lit == 0
        want, nst, _ = nc.render(pto, pto.Scene(sd), params)
        img, st, _ = ec.render(pto, pto.Scene(sd), params, env=black, flags=ec.NEE)
        assert np.array_equal(img, want) and (st.ext_rays, st.shadow_rays) == (nst.ext_rays, nst.shadow_rays), name


def moments(P, pto, osc, env, flags, spp=SPP):
    """(per-pixel mean, per-pixel sample variance of one sample's radiance, stats) of the checker at S x S."""
    params = P.make_params(S, S, spp=spp, max_depth=8, streams=1, seed=11)
    img, st, sq = ec.render(pto, osc, params, env=env, flags=flags, with_sq=True)
    m = img[..., :3].astype(np.float64)
    return m, (sq / spp - m * m) * spp / (spp - 1), st


def max_z(a, b, spp=SPP):
    """Largest |z| of the difference of two independent estimates: over the whole image and over its 8 x 8-pixel blocks, per channel
    (tests/test_nee.py's). A block without variance in either estimate — every pixel sees the environment directly, the same
    deterministic lookup in both — has to agree exactly: z = 0 there if it does, infinite if not."""
    d, v = a[0] - b[0], (a[1] + b[1]) / spp

    def z(dd, vv):
        dd, vv = np.abs(dd.sum((0, 1))), vv.sum((0, 1))
        return np.where(vv > 0, dd / np.sqrt(np.where(vv > 0, vv, 1.0)), np.where(dd == 0, 0.0, np.inf))
    zs = [z(d, v)]
    for by in range(0, S, 8):
        for bx in range(0, S, 8):
            zs.append(z(d[by:by + 8, bx:bx + 8], v[by:by + 8, bx:bx + 8]))
    return float(np.max(zs))


SCENES = ["soup", "cornell", "glass"]


COARSE = 4   # side of the coarse sun map: where s varies most inside a texel (see test_negative_controls_fail)


@pytest.fixture(scope="module")
def stat(P, pto):
    """stat(n) -> per scene the oracle scene (with the oracle's own BVH: the picture is the brute-force one), the moments of the plain
    estimator (§5 with §11's miss) under the n x n sun map and those of the NEE estimator — computed once per n, shared."""
    scenes, done = {}, {}

    def get(n):
        if n not in done:
            env = ec.sun_sky(P, n)
            for name in SCENES:
                if name not in scenes:
                    scenes[name] = pto.Scene(ec.scene(P, name, S, S, SOUP))
                    scenes[name].build_own_bvh()
            plain = {name: moments(P, pto, scenes[name], env, 0) for name in SCENES}
            assert all(p[2].shadow_rays == 0 for p in plain.values())
            done[n] = (env, scenes, {k: p[:2] for k, p in plain.items()}, {name: moments(P, pto, scenes[name], env, ec.NEE) for name in SCENES})
        return done[n]
    return get


@pytest.mark.parametrize("n", [64, COARSE])
@pytest.mark.parametrize("name", SCENES)
def test_nee_is_unbiased(stat, name, n):
    """Sampling the map (soup: the only light; Cornell and Cornell-glass: half of the light samples, the ceiling light the other half)
    leaves the mean where the plain estimator has it, within 4 sigma over the image and over blocks. Measured (soup / Cornell /
    glass): 2.5 / 2.2 / 1.4 under the 64 x 64 map, 2.2 / 1.5 / 1.4 under the 4 x 4 one."""
    _, _, plain, nee = stat(n)
    m, v, st = nee[name]
    assert st.shadow_rays > 0 and st.lit == 1 and (st.n_lights > 0) == (name != "soup")
    assert max_z((m, v), plain[name]) < Z, (name, n)


@pytest.mark.parametrize("flag,n", [(ec.NO_JACOBIAN, 64), (ec.NO_MIS, 64), (ec.NO_PSEL, 64), (ec.SAMPLED_TEXEL, COARSE)],
                         ids=["no_jacobian", "no_mis", "no_psel", "sampled_texel"])
def test_negative_controls_fail(P, pto, stat, flag, n):
    """Each deliberate error exceeds the bound on at least one of the three scenes. Measured largest |z| (soup / Cornell / glass)
    under the 64 x 64 map: s^3 dropped 69 / 143 / 97; MIS dropped 82 / 189 / 153; psel dropped 2.5 (one kind of light: psel is 1
    anyway) / 123 / 90.

    sampled_texel is what skipping §11's second lookup leads to: radiance, density AND Jacobian of the sampled texel (i, j) — its
    centre's s, i.e. the texel's own solid angle, a pdf that is constant over the texel — instead of (E, p, s) at encode(wl). (Taking
    only E and p from (i, j) and s from wl is no error to measure: decode and encode are inverses, so it is the correct estimator but
    for the one sample in 10^5 that a float rounding carries over a texel edge, and gives the correct checker's |z| to nine digits.
    The device is held to that bit-level rule by the bit-for-bit frames of tests/test_gpu_env.py.) The error is the variation of s^3
    inside a texel, which shrinks as 1 / n: largest |z| 2.5 / 2.2 / 1.5 at n = 64 (invisible), 2.1 / 2.3 / 2.0 at n = 16,
    4.2 / 5.1 / 3.3 at n = 8, 16.3 / 13.2 / 10.4 at n = 4. So this control is judged under the 4 x 4 sun map, where
    test_nee_is_unbiased holds the correct checker to the same bound."""
    env, scenes, plain, _ = stat(n)
    zs = [max_z(moments(P, pto, scenes[name], env, ec.NEE | flag)[:2], plain[name]) for name in SCENES]
    print(f"control {flag} under the {n} x {n} map: largest |z| " + " / ".join(f"{z:.2f}" for z in zs))
    assert max(zs) > Z, (flag, zs)


def test_variance_is_lower(stat):
    """On the sun-lit soup the summed per-pixel variance with NEE is below the plain one (measured: 10x)."""
    _, _, plain, nee = stat(64)
    assert nee["soup"][1].sum() < plain["soup"][1].sum()


def test_product_does_not_reference_the_checker():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "pathtracing_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".h", ".hip", "Makefile")):
                txt = open(os.path.join(dirpath, f), errors="replace").read()
                assert "env_ref" not in txt and "env_checker" not in txt and "er_render" not in txt, f
