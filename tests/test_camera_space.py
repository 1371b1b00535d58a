"""The camera space without a GPU (tests/camera_space.py has the cases): cameras that are rolled, off-centre, anisotropic, skewed,
long, left-handed, mirrored, zoomed, wide, far, shifted, sheared to the rule's threshold, or degenerate, over Cornell (BVH2), the
tessellated Cornell in layouts 68, 72 and 73, a spheres-only scene and one triangle, in 64 x 48 frames.

* §3's camera ray of the oracle against a float64 evaluation of §3, within a bound derived from the roundings of §3.
* The rule of DESIGN.md "Sky pixels: The bound", restated in float64 (camera_space.scene_rect64), is sound per the oracle alone: no
  pixel it would resolve has a sample that hits. tests/test_gpu_camera_space.py holds the device's rectangle to the same function.
* Seven deliberately wrong rules each break that soundness on some (case, scene): the cases are sharp enough.
* Few enough reference rectangles have a side on an integer for the device to be compared with them exactly."""
import numpy as np
import pytest

import camera_space as cs
import temporal_cases as tc
from float64_support import build_bvh_detached

U = 2.0 ** -24  # the unit roundoff of float32


class Prepared:
    """One (case, scene): the scene data, its blob from the host builder, the root's boxes, and the oracle's sky mask."""

    def __init__(self, P, pto, csd, layout):
        self.sd = csd
        info, nodes, tris = build_bvh_detached(csd, layout)
        self.bvh = (info.width, nodes, tris) if len(csd.tri_mat) else None
        self.slots = cs.root_slots(info.width, nodes) if len(csd.tri_mat) else []
        self.sky = cs.sky_mask(P, pto, csd, P.make_params(cs.W, cs.H, spp=256, max_depth=1), self.bvh)

    def rect(self, variant=None):
        return cs.scene_rect64(self.slots, self.sd.spheres, self.sd.cam, cs.W, cs.H, variant)


_tables, _prepared = {}, {}


def cases_of(P, name):
    """({case: scene data}, layout) of scene `name`, made once."""
    if name not in _tables:
        sd, layout = cs.scene(P, name)
        _tables[name] = (cs.cases(P, sd), layout)
    return _tables[name]


@pytest.fixture(scope="module")
def prepared(P, pto):
    """prepared(case, scene) -> Prepared, made once per module."""
    def get(case, name):
        if (case, name) not in _prepared:
            table, layout = cases_of(P, name)
            _prepared[(case, name)] = Prepared(P, pto, table[case], layout)
        return _prepared[(case, name)]
    return get


# ------------------------------------------------------------------------------------------------ §3 against float64

def angle_bound(cam, x, y):
    """First-order bound on the angle between §3's float32 direction and its exact value, from the roundings of §3 (u = 2^-24,
    jitter 0.5, so x + 0.5 is exact):

        tx = fl((x + 0.5) scale)                  |dtx| <= u |tx|
        sx = fl(tx - cx)                          |dsx| <= u |sx| + u |tx|                                (likewise sy, ty)
        i_k = fl(sx right_k + forward_k)          one rounding of the fma: <= u (|sx| |right_k| + |forward_k|), plus |dsx| |right_k|
        v_k = fl(sy up_k + i_k)                   one rounding: <= u (|sx| |right_k| + |sy| |up_k| + |forward_k|), plus |dsy| |up_k|

        |dv_k| <= E_k = u ((3 |sx| + |tx|) |right_k| + (2 |sy| + |ty|) |up_k| + 2 |forward_k|)

    With |tx| <= |sx| + |cx| that is at most 4 m_k + u (|cx| |right_k| + |cy| |up_k|) for m_k = u (|sx| |right_k| + |sy| |up_k| +
    |forward_k|): four of the units m_k / |v|, and the cancellation in tx - cx, which only a camera whose principal point is far from
    the pixel pays (zoom_edge, the threshold cameras). normalize multiplies every component by the same s, whose own error (three
    roundings in the dot product, the square root, the reciprocal) turns nothing; the three products v_k s add one rounding each,
    a vector of length <= u |d|. So

        angle <= |E| / |v| + u,                   taken times 1 + 2^-10 for the second-order terms.

    Returns (bound, the unit |m| / |v|)."""
    c = cs.Cam64(cam)
    v, (sx, sy, tx, ty) = cs.camera_dir64(cam, x, y)
    r, u, f = np.abs(c.r), np.abs(c.u), np.abs(c.f)
    E = U * ((3 * abs(sx) + abs(tx)) * r + (2 * abs(sy) + abs(ty)) * u + 2 * f)
    m = U * (abs(sx) * r + abs(sy) * u + f)
    n = np.linalg.norm(v)
    return (np.linalg.norm(E) / n + U) * (1 + 2.0 ** -10), np.linalg.norm(m) / n


@pytest.mark.parametrize("case", cs.CASE_NAMES)
def test_camera_ray_against_float64(P, pto, case):
    """pto.camera_ray at the four corner pixels, the centre and 200 random pixels of every scene's camera of the case, at jitter 0.5
    (the camera's jitter flag off: §3's jx = jy = 0.5f), against §3 in float64 on the same float32 words: the angle stays within
    angle_bound, whose docstring has the derivation; the origin is the camera's, bit for bit; |d| = 1 within 4.5 u (the dot product's
    three roundings, halved by the square root: 1.5 u; one each for the square root, the reciprocal and the product).

    Measured, the largest angle per case as a share of its bound, and in the units 2^-24 |m| / |v| of the bound's leading term (the
    bound is four of them plus the cancellation term plus u): default, long_forward, shifted_world, no_jitter, inside, behind 0.301
    (1.04 units); rolled 0.257 (0.89); off_centre 0.378 (1.47); anisotropic 0.364 (1.58); skewed 0.228 (0.87); narrow 0.043 (0.13);
    left_handed 0.226 (0.80); mirrored 0.303 (1.07); zoom_edge 0.165 (0.52); wide, beside_wide 0.318 (1.97); far 0.002 (0.005: forward
    dominates v); corner_on_threshold_in 0.110 (0.28), _out 0.108 (0.27); beside_plane 0.259 (1.00); scale_zero 0.073 (0.24);
    scale_negative 0.324 (1.24); flat_basis 0.252 (1.00). No case exceeds 0.38 of its bound or two units."""
    rng = np.random.default_rng(3)
    pixels = [(0, 0), (cs.W - 1, 0), (0, cs.H - 1), (cs.W - 1, cs.H - 1), (cs.W // 2, cs.H // 2)]
    pixels += list(zip(rng.integers(0, cs.W, 200).tolist(), rng.integers(0, cs.H, 200).tolist()))
    share, units = 0.0, 0.0
    for name in cs.SCENES:
        cam = tc.copy_camera(cases_of(P, name)[0][case].cam)
        cam.jitter = 0
        for x, y in pixels:
            o, d = pto.camera_ray(cam, x, y)
            v, _ = cs.camera_dir64(cam, x, y)
            assert np.array_equal(o, np.array(cam.origin[:], np.float32))
            d64 = d.astype(np.float64)
            angle = np.arctan2(np.linalg.norm(np.cross(d64, v)), np.dot(d64, v))
            bound, unit = angle_bound(cam, x, y)
            assert angle <= bound, (case, name, x, y, angle, bound)
            assert abs(np.linalg.norm(d64) - 1.0) <= 4.5 * U, (case, name, x, y, np.linalg.norm(d64))
            share, units = max(share, angle / bound), max(units, angle / unit)
    print(f"camera ray {case}: largest angle {share:.3f} of the bound, {units:.3f} units")


# ------------------------------------------------------------------------------------------------ the rule is sound

@pytest.mark.parametrize("case", cs.CASE_NAMES)
def test_rule_is_sound_per_the_oracle(prepared, case):
    """The oracle's frame at max_depth = 1 and 256 spp, jitter as the case says, and the same frame of the empty scene: a pixel equals
    the empty frame's exactly if and only if all 256 samples missed. Every pixel outside scene_rect64 is such a pixel. The resolving
    cases have both kinds of pixel (between 2 % and 98 % sky); the give-up cases return None."""
    for name in cs.SCENES:
        p = prepared(case, name)
        result, sides = p.rect()
        bad = cs.unsound(result, p.sky)
        assert len(bad) == 0, (case, name, result, len(bad), bad[:4].tolist())
        if case in cs.GIVE_UP:
            assert result is None and sides is None, (case, name, result)
        else:
            assert 0.02 < p.sky.mean() < 0.98, (case, name, p.sky.mean())
            assert sides is not None, (case, name)


def test_the_rule_resolves_pixels_in_every_resolving_case(prepared):
    """Sound because the margins hold, not because the rule gave up: every resolving case yields a rectangle that leaves pixels out on
    some scene, and every scene has one in at least eight cases."""
    for case in cs.RESOLVING:
        assert any(isinstance(prepared(case, name).rect()[0], tuple) for name in cs.SCENES), case
    for name in cs.SCENES:
        assert sum(isinstance(prepared(case, name).rect()[0], tuple) for case in cs.RESOLVING) >= 8, name


# ------------------------------------------------------------------------------------------------ negative controls

@pytest.mark.parametrize("variant", cs.VARIANTS)
def test_wrong_rules_are_unsound_somewhere(prepared, variant):
    """Each deliberately wrong variant of scene_rect64 would resolve a pixel that the oracle shows hit, on at least one (case, scene)."""
    caught = [(case, name) for case in cs.CASE_NAMES for name in cs.SCENES
              if len(cs.unsound(prepared(case, name).rect(variant)[0], prepared(case, name).sky))]
    print(f"{variant}: unsound on {len(caught)} (case, scene) pairs, first {caught[:5]}")
    assert caught, variant


# ------------------------------------------------------------------------------------------------ ties

def test_few_rectangles_have_a_side_on_an_integer(prepared):
    """tests/test_gpu_camera_space.py compares the device's rectangle with scene_rect64's exactly, which is fair only where no
    real-valued side lies within 1e-6 of an integer: at most one (case, scene) in ten may be left out for that. Measured: 0 of 138."""
    pairs = [(case, name) for case in cs.CASE_NAMES for name in cs.SCENES]
    left_out = [k for k in pairs if cs.tied(prepared(*k).rect()[1], cs.W, cs.H)]
    print(f"sides on an integer: {len(left_out)} of {len(pairs)} (case, scene) pairs {left_out}")
    assert len(left_out) <= 0.1 * len(pairs), left_out
