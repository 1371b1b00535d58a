"""Albedo textures (docs/SPEC.md §13) across the texture and UV space without a GPU: the scalar checker of tests/tex_ref/, which the
device is held to bit for bit, against float64 (tests/tex64.py has §13's meaning in float64 and the derived bound,
tests/texture_space.py the cases, the probe scene and the judgement; its conditions on the space are asserted when it is imported).

* For every size x filter x contents x family, at the barycentrics of the probe's camera rays: a bilinear lookup within tol of the
  float64 interpolation at every near point, a nearest lookup one of the float64 candidates bit for bit, every lookup finite and inside
  the texture's envelope, a one-colour texture's colour exactly. A bit-for-bit comparison with an f32 restatement cannot see a formula
  that is wrong in both; this one does (a half-texel shift, a clamp for a repeat, swapped vertices, a flipped row).
* What the coordinate means: with UVs an affine function of the place on the wall, the float64 interpolation at the float64 hit point
  of tests/ray_caster64.py — which vertex carries which UV, and that row 0 is t = 0."""
import numpy as np
import pytest

import ray_caster64 as rc
import tex64
import tex_checker as tc
import texture_space as ts

BARYCENTRIC_BOUND = 1e-4  # test_gpu_trace.test_barycentrics: an f32 (u, v) against float64


@pytest.fixture(scope="module")
def rays(P, pto):
    """The probe's camera rays that hit the wall, once: (pixels, triangle ids, u, v as the checker's §4 gives them, float64 hit points).
    The ids are the float64 caster's, and they are the ones texture_space's own float64 camera expects."""
    sheet = ts.probe((3, 5), "distinct", "unit", 0)
    sd = sheet.scene(P)
    o, d = rc.camera_rays(pto, sd.cam, ts.W, ts.H)
    ids, t, _, _ = rc.cast(sd.verts, sd.spheres, o, d)
    px = np.nonzero(ids != rc.MISS)[0]
    assert np.array_equal(px, ts.IDEAL[0]) and np.array_equal(ids[px].astype(np.int64), ts.IDEAL[1])
    u, v = tc.barycentrics_many(sd.verts[ids[px].astype(np.int64)], o[px], d[px])
    assert np.abs(u - ts.IDEAL[2]).max() <= BARYCENTRIC_BOUND and np.abs(v - ts.IDEAL[3]).max() <= BARYCENTRIC_BOUND
    hit = o[px].astype(np.float64) + t[px, None] * d[px].astype(np.float64)
    return px, ids[px].astype(np.int64), u, v, hit


@pytest.mark.parametrize("filter_name", list(ts.FILTERS))
@pytest.mark.parametrize("family", ts.FAMILIES)
def test_checker_against_float64(rays, family, filter_name):
    px, ids, u, v, _ = rays
    for size in ts.SIZES:
        worst = 0.0
        for contents in ts.CONTENTS:
            sheet = ts.probe(size, contents, family, ts.FILTERS[filter_name])
            got = ts.checker_texels(sheet, ids, u, v)
            res = ts.hold(sheet, ids, u, v, got, (family, filter_name, size, contents))
            worst = max(worst, res[ts.SUBJECT][0])
            meant = ts.stated(size, contents, family)
            if filter_name == "bilinear" and meant == "near" and family != "constants":
                assert res[ts.SUBJECT][1] == res[ts.SUBJECT][2], (family, size, contents, "a near case with far points", res[ts.SUBJECT])
            if filter_name == "bilinear" and family == "constants" and meant != "exact" and contents != "hdr":
                assert res[ts.SUBJECT][1] >= 0.6 * res[ts.SUBJECT][2], (size, contents, res[ts.SUBJECT])
        if filter_name == "bilinear":
            print(f"checker {family} {size[0]}x{size[1]}: largest err / tol {worst:.3f}")


def test_the_tile_wall_reaches_the_edges(rays):
    """What `constants` is there for, seen in the checker's own f32 coordinates: s - floorf(s) == 1.0f and the value just below it,
    2^20 and -2^20 themselves, a coordinate on a texel border, and pixels with more than one candidate texel."""
    px, ids, u, v, _ = rays
    for size in ((3, 5), (255, 257)):
        sheet = ts.probe(size, "distinct", "constants", tc.NEAREST)
        sub = sheet.tile_texture[ids // 2] == ts.SUBJECT
        q = sheet.uvs[ids[sub]]
        _, st = tc.lookup_many(sheet.textures[ts.SUBJECT].img, q, u[sub], v[sub], tc.NEAREST)
        for axis, n in ((0, size[0]), (1, size[1])):
            c = st[:, axis]
            f = c - np.floor(c)  # f32, as §13 wraps
            assert (f == np.float32(1.0)).any() and (c == np.float32(2.0 ** 20)).any() and (c == np.float32(-2.0 ** 20)).any(), (size, axis)
            # (1 - 2^-24: its product with n never rounds up to n, W 2^-24 being more than half an ulp below W)
            assert (f == np.float32(1.0 - 2.0 ** -24)).any(), (size, axis)
            border = q[:, axis] == np.float32((n // 2) / n)
            x = f[border].astype(np.float64) * n
            assert (np.floor(x) == n // 2).any() and ((np.floor(x) == n // 2 - 1).any() or x.min() == n // 2), (size, axis, x.min(), x.max())
        s, t = tex64.coordinate(q, u[sub], v[sub])
        _, dx, dy = tex64.bound(sheet.textures[ts.SUBJECT].stats, q)
        assert (tex64.nearest_candidates(sheet.textures[ts.SUBJECT].img, s, t, dx, dy).count > 1).any()


@pytest.mark.parametrize("family", [f for f in ts.FAMILIES if f != "constants"])
def test_the_coordinate_means_the_hit_point(rays, family):
    """The checker's lookup at its own f32 barycentrics against the float64 interpolation at the family's (s, t) of the float64 hit
    point. The bound is tol widened by what the two coordinates may differ by, times W Dx + H Dy: the barycentrics' 1e-4 times the
    triangle's UV span, and e S for the vertices' UVs, which are the family's rounded to f32."""
    px, ids, u, v, hit = rays
    a, b = ts.wall_place(hit[:, :2])
    judged = 0
    for size in ts.SIZES:
        A, c = ts.affine(family, size)
        s, t = A[0, 0] * a + A[0, 1] * b + c[0], A[1, 0] * a + A[1, 1] * b + c[1]
        q = ts.uvs(size, family)[ids].astype(np.float64).reshape(-1, 3, 2)
        span = (q.max(1) - q.min(1)).max(1)
        extra = BARYCENTRIC_BOUND * span + tex64.E * np.abs(q).max((1, 2))
        for contents in ("distinct", "checker"):
            sheet = ts.probe(size, contents, family, 0)
            got = ts.checker_texels(sheet, ids, u, v)
            res = ts.hold(sheet, ids, u, v, got, (family, size, contents, "hit point"), extra=extra, only=ts.SUBJECT, st=(s, t))
            # every point is judged where the widened bound is still small: 3 x 5 always, 63 x 65 under a span below one repeat
            if (size == (3, 5) or (size == (63, 65) and family != "minified")) and not family.startswith(("offset", "neg_offset")):
                assert res[ts.SUBJECT][1] == res[ts.SUBJECT][2], (family, size, contents, res[ts.SUBJECT])
            judged += res[ts.SUBJECT][1]
    assert judged > 0
