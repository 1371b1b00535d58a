"""The thin-lens camera (docs/SPEC.md §3.1) without a GPU: the scalar checker of tests/lens_ref/ against the oracle where there is no lens,
against geometry where there is one (the focal plane stays sharp, a point off it becomes a uniform disc of the predicted radius that
carries the pinhole's flux), the host rules of pt_scene_set_lens on a detached scene, and pipeline.h's decode with its lens parameter.

The device is held to the checker bit for bit by tests/test_gpu_lens.py."""
import ctypes as C
import itertools

import numpy as np
import pytest

import lens_checker as lc
import nee_checker as nc
import pipeline_checker as pc
import pipelines as pl

W, H = 48, 36
SCALE = 1.0 / 32.0
Z = 4.0  # the statistical tests' bound, in standard errors


def pixel_to_world(px, py, depth):
    """The point at `depth` in front of lc.camera(P, W, H) that a pinhole projects to image position (px, py), in pixels."""
    return ((px * SCALE - 0.5 * W * SCALE) * depth, (py * SCALE - 0.5 * H * SCALE) * depth, -depth)


def triangle_at(pixels, depth):
    return [c for px, py in pixels for c in pixel_to_world(px, py, depth)]


# ------------------------------------------------------------------------------------------------- convex polygons in the image plane (float64)
def _axes(poly):
    e = np.roll(poly, -1, axis=0) - poly
    return np.stack([-e[:, 1], e[:, 0]], 1)


def _disjoint(a, b):
    """Separating axis theorem: whether the convex polygons a and b (k x 2) have no point in common."""
    for ax in np.concatenate([_axes(a), _axes(b)]):
        pa, pb = a @ ax, b @ ax
        if pa.max() < pb.min() or pb.max() < pa.min():
            return True
    return False


def _inside(poly, pts):
    """Whether every point of pts lies inside the convex polygon poly (either orientation)."""
    e = np.roll(poly, -1, axis=0) - poly
    s = np.array([[e[i, 0] * (p[1] - poly[i, 1]) - e[i, 1] * (p[0] - poly[i, 0]) for i in range(len(poly))] for p in pts])
    return bool((s >= 0).all() or (s <= 0).all())


def _seg_dist(p, a, b):
    ab = b - a
    t = np.clip(np.dot(p - a, ab) / np.dot(ab, ab), 0.0, 1.0)
    return float(np.linalg.norm(p - (a + t * ab)))


def _distance(a, b):
    """The distance between the convex polygons a and b; 0 where they meet."""
    if not _disjoint(a, b):
        return 0.0
    d = [_seg_dist(p, q[i], q[(i + 1) % len(q)]) for p_set, q in ((a, b), (b, a)) for p in p_set for i in range(len(q))]
    return min(d)


def _square(x, y, grow):
    return np.array([[x - grow, y - grow], [x + 1 + grow, y - grow], [x + 1 + grow, y + 1 + grow], [x - grow, y + 1 + grow]], np.float64)


# ------------------------------------------------------------------------------------------------------------------------ 1. pinhole limit
@pytest.mark.parametrize("kind", ["PT_SCENE_CORNELL_GLASS", "PT_SCENE_CORNELL"])
def test_pinhole_limit(P, pto, kind):
    """No lens, and a lens of radius 0: pto_render bit for bit (rays too); with LR_NEE, nr_render."""
    sd = P.make_scene(getattr(P.native, kind), 0, 3, W, H)
    osc = pto.Scene(sd)
    p = P.make_params(W, H, spp=5, streams=2, max_depth=6, rr_start=2)
    want, ost = pto.render(osc, p)
    nee_want, nst, _ = nc.render(pto, osc, p)
    for lens in (None, (0.0, 3.0)):
        got, st, _ = lc.render(pto, osc, p, lens=lens)
        assert np.array_equal(got, want) and st.ext_rays == ost.rays and st.paths == ost.paths and st.shadow_rays == 0
        got, st, _ = lc.render(pto, osc, p, lens=lens, flags=lc.NEE)
        assert np.array_equal(got, nee_want) and (st.ext_rays, st.shadow_rays) == (nst.ext_rays, nst.shadow_rays) and st.shadow_rays > 0
    through, _, _ = lc.render(pto, osc, p, lens=(0.05, 2.5))
    assert not np.array_equal(through, want)  # the comparisons above are not vacuous: a lens changes the frame


# -------------------------------------------------------------------------------------------------------------------------- 2. focal plane
FOCUS, FOCAL_RADIUS = 2.0, 0.1
FOCAL_TRI = [(5.3, 4.2), (43.7, 9.6), (20.4, 32.9)]  # in pixels; large, so that few pixels touch an edge


def _focal_frames(P, pto, jitter, flags=0):
    sd = lc.triangle_scene(P, W, H, triangle_at(FOCAL_TRI, FOCUS), lc.camera(P, W, H, scale=SCALE, jitter=jitter))
    osc = pto.Scene(sd)
    p = P.make_params(W, H, spp=8, streams=1, max_depth=1)
    pin, _ = pto.render(osc, p)
    lens, _, _ = lc.render(pto, osc, p, lens=(FOCAL_RADIUS, FOCUS), flags=flags)
    return pin, lens


def _clear_pixels():
    """The pixels whose footprint on the focal plane, grown by 1/64 pixel, lies wholly inside or wholly outside the triangle."""
    tri = np.array(FOCAL_TRI, np.float64)
    clear = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            sq = _square(x, y, 1.0 / 64.0)
            clear[y, x] = _inside(tri, sq) or _disjoint(tri, sq)
    return clear


@pytest.mark.parametrize("jitter", [0, 1])
def test_the_focal_plane_is_sharp(P, pto, jitter):
    """A triangle in the plane through origin + F forward: every lens ray of a sample meets that plane where the pinhole ray does, so a
    pixel that lies clear of the triangle's edges is the pinhole frame's, exactly. LR_FOCUS_IGNORED blurs the edges by up to
    R / (F scale) = 1.6 pixels and fails."""
    clear = _clear_pixels()
    assert (~clear).sum() <= W * H // 4, int((~clear).sum())
    pin, lens = _focal_frames(P, pto, jitter)
    assert np.array_equal(lens[clear], pin[clear])
    assert (pin[clear][:, 0] > 0).any() and (pin[clear][:, 0] == 0).any()  # pixels on both sides of the edges
    _, wrong = _focal_frames(P, pto, jitter, lc.FOCUS_IGNORED)
    assert not np.array_equal(wrong[clear], pin[clear])


# ----------------------------------------------------------------------------------------------------------------- 3. circle of confusion
# A triangle of half a square pixel at depth ZD, seen through a lens focused at CF: a point there is imaged as a disc of radius
# RHO = R |1 / ZD - 1 / CF| / scale pixels around its pinhole image. ZD << CF, so that LR_FIXED_ORIGIN — which turns the ray at the
# pinhole and blurs by R / (CF scale) = 0.4 pixels — is far from it.
ZD, CF, RHO = 0.5, 8.0, 6.0
COC_RADIUS = RHO * SCALE / abs(1.0 / ZD - 1.0 / CF)
COC_TRI = [(23.8, 17.9), (24.8, 17.9), (23.8, 18.9)]
CENTROID = np.mean(np.array(COC_TRI, np.float64), axis=0)


def _coc_scene(P, pto):
    return pto.Scene(lc.triangle_scene(P, W, H, triangle_at(COC_TRI, ZD), lc.camera(P, W, H, scale=SCALE, jitter=1)))


def _centre_distance():
    yy, xx = np.mgrid[0:H, 0:W]
    return np.hypot(xx + 0.5 - CENTROID[0], yy + 0.5 - CENTROID[1])


def test_the_circle_of_confusion_has_the_predicted_radius(P, pto):
    """Outside: a pixel whose footprint, grown by RHO + 1/64 pixel, misses the triangle is exactly 0. Inside: every pixel whose centre is
    within RHO / 2 of the centroid's image is lit — at 4096 spp. A sample of such a pixel hits the triangle with probability
    area / (pi RHO^2) = 0.5 / 113 = 0.0044, so at 64 spp a pixel stays black with probability 0.75 under the correct rule; at 4096 it
    does with 1.4e-8, and the 28 pixels are all lit. LR_FIXED_ORIGIN lights a patch of 0.4 + the triangle's own size and fails."""
    assert abs(RHO - 6.0) < 1e-9 and CENTROID[0] - RHO - 2 > 0 and CENTROID[1] + RHO + 2 < H
    osc = _coc_scene(P, pto)
    p = P.make_params(W, H, spp=4096, streams=1, max_depth=1)
    img, _, _ = lc.render(pto, osc, p, lens=(COC_RADIUS, CF))
    tri = np.array(COC_TRI, np.float64)
    far = np.array([[_distance(tri, _square(x, y, 0.0)) > RHO + 1.0 / 64.0 for x in range(W)] for y in range(H)])
    assert far.sum() > W * H // 2 and (img[far][:, :3] == 0).all()
    near = _centre_distance() <= RHO / 2
    assert near.sum() >= 24 and (img[near][:, 0] > 0).all(), int((img[near][:, 0] > 0).sum())
    lit_radius = _centre_distance()[img[..., 0] > 0].max()
    assert lit_radius > RHO - 1.5, lit_radius  # the disc is filled to its rim, not only at its centre
    wrong, _, _ = lc.render(pto, osc, p, lens=(COC_RADIUS, CF), flags=lc.FIXED_ORIGIN)
    assert not (wrong[near][:, 0] > 0).all()


# ---------------------------------------------------------------------------------------------- 4. uniform aperture and conserved flux
def _sum_and_error(img, sq, n, mask=None):
    """(sum over the masked pixels of the red channel's mean, its standard error) from the per-pixel sums of squares of n samples."""
    m = np.ones(img.shape[:2], bool) if mask is None else mask
    mean = img[..., 0].astype(np.float64)[m]
    var_of_mean = np.maximum(sq[..., 0][m] / n - mean * mean, 0.0) / n
    return float(mean.sum()), float(np.sqrt(var_of_mean.sum()))


def test_the_aperture_is_uniform_and_conserves_flux(P, pto):
    """256 spp with jitter. The image sum is the pinhole frame's within 4 standard errors (the disc lies inside the image); the mean of
    the pixels within 0.4 RHO of the centre is the mean of the ring 0.6 RHO .. 0.9 RHO, to the same criterion. LR_LINEAR_RADIUS
    (r = u: a density that falls as 1 / r) fails the ring comparison.
    z-scores seen with this seed: image sum 1.44; centre against ring 0.22 under the rule, 5.37 under LR_LINEAR_RADIUS."""
    n = 256
    osc = _coc_scene(P, pto)
    p = P.make_params(W, H, spp=n, streams=1, max_depth=1)
    pin, _, pin_sq = lc.render(pto, osc, p, lens=None, with_sq=True)
    dist = _centre_distance()
    inner, ring = dist <= 0.4 * RHO, (dist >= 0.6 * RHO) & (dist <= 0.9 * RHO)

    def z_of(flags):
        img, _, sq = lc.render(pto, osc, p, lens=(COC_RADIUS, CF), flags=flags, with_sq=True)
        a, ea = _sum_and_error(img, sq, n, inner)
        b, eb = _sum_and_error(img, sq, n, ring)
        a, ea, b, eb = a / inner.sum(), ea / inner.sum(), b / ring.sum(), eb / ring.sum()
        return img, sq, abs(a - b) / np.hypot(ea, eb)

    img, sq, z_ring = z_of(0)
    s0, e0 = _sum_and_error(pin, pin_sq, n)
    s1, e1 = _sum_and_error(img, sq, n)
    z_sum = abs(s1 - s0) / np.hypot(e0, e1)
    _, _, z_wrong = z_of(lc.LINEAR_RADIUS)
    print(f"z-scores: image sum {z_sum:.2f}; centre against ring {z_ring:.2f}, with LR_LINEAR_RADIUS {z_wrong:.2f}")
    assert s0 > 0 and e0 > 0 and e1 > 0
    assert z_sum < Z, z_sum
    assert z_ring < Z, z_ring
    assert z_wrong > Z, z_wrong


# ---------------------------------------------------------------------------------------------------------- 5. host rules without a device
def _ulp_distance(a, b):
    ia, ib = (np.asarray(v, np.float32).view(np.int32).astype(np.int64) for v in (a, b))
    ia, ib = (np.where(i < 0, -(i & 0x7FFFFFFF), i) for i in (ia, ib))
    return np.abs(ia - ib)


def test_lens_basis_against_float64(P, pto):
    rng = np.random.default_rng(11)
    for k in range(200):
        cam = lc.camera(P, W, H)
        right, up = rng.normal(size=3) * 10.0 ** rng.uniform(-3, 3), rng.normal(size=3) * 10.0 ** rng.uniform(-3, 3)
        cam.right[:], cam.up[:] = right.tolist(), up.tolist()
        radius = float(np.float32(10.0 ** rng.uniform(-3, 1)))
        u, v = lc.lens_basis(pto, cam, radius)
        for got, axis in ((u, cam.right), (v, cam.up)):
            a = np.array(axis[:], np.float64)
            want = radius * a / np.linalg.norm(a)
            assert (_ulp_distance(got, want.astype(np.float32)) <= 2).all(), (k, got, want)
    flat = lc.camera(P, W, H)
    flat.up[:] = (0.0, 0.0, 0.0)
    assert lc.lens_basis(pto, flat, 0.5) is None
    tiny = lc.camera(P, W, H)
    tiny.right[:] = (1e-30, 0.0, 0.0)  # dot(right, right) underflows to 0
    assert lc.lens_basis(pto, tiny, 0.5) is None


def test_set_get_clear_on_a_detached_scene(P):
    N = P.native
    s = C.c_void_p()
    assert N.lib.pt_scene_create(None, C.byref(s)) == 0
    try:
        def get():
            out = N.pt_lens(radius=-1.0, focus_distance=-1.0, flags=7)
            assert N.lib.pt_scene_get_lens(s, C.byref(out)) == 0 and out.flags == 0 and list(out.pad) == [0] * 5
            return out.radius, out.focus_distance

        def put(radius, focus, flags=0):
            return N.lib.pt_scene_set_lens(s, C.byref(N.pt_lens(radius=radius, focus_distance=focus, flags=flags)))

        assert get() == (0.0, 0.0)
        assert put(0.25, 3.5) == 0 and get() == (0.25, 3.5)
        bad = N.PT_ERR_INVALID_ARGUMENT
        for radius, focus, flags in ((-0.5, 1.0, 0), (np.nan, 1.0, 0), (np.inf, 1.0, 0), (-np.inf, 1.0, 0), (0.5, 0.0, 0), (0.5, -2.0, 0),
                                     (0.5, np.nan, 0), (0.5, np.inf, 0), (0.5, 1.0, 1), (0.5, 1.0, 0x80000000)):
            assert put(radius, focus, flags) == bad, (radius, focus, flags)
            assert b"pt_scene_set_lens" in N.lib.pt_last_error(None)
            assert get() == (0.25, 3.5)  # a refused value keeps the previous lens
        assert put(0.0, 1.0) == 0 and get() == (0.0, 1.0)   # radius 0 is a valid lens: the pinhole
        assert put(0.5, 2.0) == 0 and N.lib.pt_scene_set_lens(s, None) == 0 and get() == (0.0, 0.0)
        assert N.lib.pt_scene_set_lens(None, None) == bad and N.lib.pt_scene_get_lens(s, None) == bad
    finally:
        N.lib.pt_scene_destroy(s)


# --------------------------------------------------------------------------------------------------------------------------- 6. pipeline
F = pl.FLAGS
BITS = [F[n] for n in ("PROFILE_KERNELS", "COUNT_VISITS", "EXTEND_PACKED", "EXTEND_SIMPLE", "BUCKET_SPECULAR", "SPLIT_KERNELS", "EXTEND_POOL",
                       "NEXT_EVENT")]
SIMPLE, PACKED, POOL = pl.EXT_SIMPLE, pl.EXT_PACKED, pl.EXT_POOL
SHADE_INLINE = 2
FIELDS = ("status", "message", "forced", "profile", "count", "split", "bucket", "nee", "env", "shade", "fuse", "full_state", "resolves_sky",
          "instrumented")


def _inputs():
    for bits in itertools.product((0, 1), repeat=len(BITS)):
        flags = sum(b for b, on in zip(BITS, bits) if on)
        for tuned, env, spec in itertools.product(range(4), (False, True), (False, True)):
            yield flags, tuned, env, spec


def _lists(d):
    return [int(x) for x in d.single_loop], [int(x) for x in d.generate_mode], [list(r) for r in d.kernel_for]


def test_the_decode_with_a_lens():
    """Every (flags, tuned kernel, environment, specular) input. Without a lens: the existing form's outputs. With one: refused exactly
    where an environment frame is (the environment's own refusal first), else the one-ray-per-lane kernel with all-kinds shading and no
    sky resolve; and what an accepted frame launches is an instantiation that exists."""
    lib = lc.build_pipeline()
    refused = accepted = 0
    for flags, tuned, env, spec in _inputs():
        ctx = (flags, tuned, env, spec)
        old, same = pc.decode(flags, tuned, env, spec), lc.decode(flags, tuned, env, spec, lens=False)
        assert all(getattr(old, k) == getattr(same, k) for k in FIELDS) and _lists(old) == _lists(same) and same.lens == 0, ctx
        d = lc.decode(flags, tuned, env, spec, lens=True)
        count = bool(flags & F["COUNT_VISITS"])
        split = bool(flags & (F["BUCKET_SPECULAR"] | F["SPLIT_KERNELS"]))
        forced = POOL if flags & F["EXTEND_POOL"] else PACKED if flags & F["EXTEND_PACKED"] else SIMPLE if flags & F["EXTEND_SIMPLE"] else tuned
        if split or count or forced in (PACKED, POOL):
            refused += 1
            assert d.status == pl.PT_ERR_UNSUPPORTED, ctx
            assert (b"environment map" in d.message) if env else (b"lens" in d.message and b"pt_scene_set_lens" in d.message), ctx
            continue
        accepted += 1
        profile, nee = bool(flags & F["PROFILE_KERNELS"]), bool(flags & F["NEXT_EVENT"])
        assert d.status == 0 and d.message is None, ctx
        assert (d.forced, d.lens, d.env, d.nee, d.count, d.split, d.bucket, d.profile) == (SIMPLE, 1, env, nee, 0, 0, 0, profile), ctx
        assert (d.shade, d.fuse, d.full_state, d.resolves_sky, d.instrumented) == (SHADE_INLINE, SHADE_INLINE, 0, 0, profile), ctx
        assert _lists(d)[0] == [int(profile), 1] and _lists(d)[1] == [0, 2], ctx
        for kernel in d.kernel_for[d.forced]:
            assert kernel == SIMPLE and lib.lp_extend_instantiated(kernel, d.fuse, d.count, d.nee, d.env, 1), ctx
    assert refused + accepted == 4096 and refused > 0 and accepted > 0
    yes = [t for t in itertools.product((1, 2, 3), (-1, 0, 1, 2), (0, 1), (0, 1), (0, 1)) if lib.lp_extend_instantiated(*t, 1)]
    assert sorted(yes) == [(SIMPLE, SHADE_INLINE, 0, n, e) for n in (0, 1) for e in (0, 1)]  # exactly 4 lens instantiations
    without = [t for t in itertools.product((1, 2, 3), (-1, 0, 2), (0, 1), (0, 1), (0, 1)) if lib.lp_extend_instantiated(*t, 0)]
    assert len(without) == 20 and len(without) + len(yes) == 24  # 20: the count tests/test_pipeline.py holds the five-argument form to
