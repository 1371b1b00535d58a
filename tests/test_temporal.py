"""pt_denoise_temporal (docs/SPEC.md §9) without a GPU: the scalar checker of tests/temporal_ref/ against float64 numpy — the running mean
of a still camera, the reprojection geometry, exactness where bilinear history must reproduce the frame, disocclusion, the quality it
buys — each wrong variant of the checker shown to break one of them, and the API's plumbing (struct layout, argument checks that need
no device).

The device is held to the checker bit for bit by tests/test_gpu_temporal.py."""
import ctypes as C

import numpy as np
import pytest

import camera_space as cs
import denoise_checker as dc
import temporal_cases as tc
import temporal_checker as tr


def hit_guides(h, w, t=2.0):
    """Every pixel a hit of primitive 0 at depth t along its ray, the normal facing the axis camera."""
    g = np.zeros((h, w, 8), np.float32)
    g[..., 0:3], g[..., 3], g[..., 4:7] = (0.0, 0.0, 1.0), t, 0.5
    return g


def random_frames(n, h, w, seed):
    rng = np.random.default_rng(seed)
    return [rng.uniform(0.0, 4.0, (h, w, 4)).astype(np.float32) for _ in range(n)]


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def test_defaults():
    assert tr.defaults() == (32, 2.0 ** -7, 0.875)


def test_still_camera_is_the_running_mean(P):
    """12 random images over fixed hit guides, max_history = 64: after call k every length is k and the image is the float64 mean of the
    k frames within 1e-5 max|c| (12 fused blends of relative error <= 2^-23 each); alpha is the frame's."""
    h, w = 9, 13
    g, cam = hit_guides(h, w), tc.axis_camera(P, w, h)
    frames = random_frames(12, h, w, 1)
    hist, total = None, np.zeros((h, w, 3))
    for k, c in enumerate(frames, 1):
        res = tr.accumulate(c, g, cam, hist, tr.params(64))
        hist = res.history
        total += c[..., :3]
        assert (res.length == k).all(), k
        assert res.taken == (w * h if k > 1 else 0)
        assert np.abs(res.image[..., :3] - total / k).max() <= 1e-5 * max(np.abs(f).max() for f in frames[:k]), k
        assert same_bits(res.image[..., 3], c[..., 3])
        assert same_bits(hist.h[..., :3], res.image[..., :3]) and same_bits(hist.h[..., 3], res.length)


def test_still_camera_max_history_is_an_exponential_average(P):
    h, w = 6, 7
    g, cam = hit_guides(h, w), tc.axis_camera(P, w, h)
    frames = random_frames(12, h, w, 2)
    hist, ref = None, None
    for k, c in enumerate(frames, 1):
        res = tr.accumulate(c, g, cam, hist, tr.params(4))
        hist = res.history
        ref = c[..., :3].astype(np.float64) if ref is None else ref + (c[..., :3] - ref) / min(k, 4)
        assert (res.length == min(k, 4)).all(), k
        assert np.abs(res.image[..., :3] - ref).max() <= 1e-5 * 4.0, k


def test_no_history(P):
    """max_history = 1, PT_TEMPORAL_RESET or a history of another size: out == c bit for bit and l == 1."""
    h, w = 6, 7
    g, cam = hit_guides(h, w), tc.axis_camera(P, w, h)
    a, b = random_frames(2, h, w, 3)
    first = tr.accumulate(a, g, cam, None)
    assert same_bits(first.image, a) and (first.length == 1).all() and first.taken == 0
    assert (tr.accumulate(b, g, cam, first.history).length == 2).all()  # the control: this history is taken
    for p in (tr.params(1), tr.params(flags=tr.RESET)):
        res = tr.accumulate(b, g, cam, first.history, p)
        assert same_bits(res.image, b) and (res.length == 1).all() and res.taken == 0
    small = tr.accumulate(a[:4, :5], hit_guides(4, 5), tc.axis_camera(P, 5, 4), None)
    res = tr.accumulate(b, g, cam, small.history)
    assert same_bits(res.image, b) and (res.length == 1).all()


def test_misses_never_accumulate(P):
    h, w = 5, 8
    g, cam = hit_guides(h, w), tc.axis_camera(P, w, h)
    g[:, 4:, 0:4] = (0.0, 0.0, 0.0, np.inf)
    g[:, 4:, 4:7] = 0.0
    g[:, 4:, 7] = np.array([tr.MISS], np.uint32).view(np.float32)[0]
    a, b = random_frames(2, h, w, 4)
    res = tr.accumulate(b, g, cam, tr.accumulate(a, g, cam).history)
    assert (res.length[:, :4] == 2).all() and (res.length[:, 4:] == 1).all() and same_bits(res.image[:, 4:], b[:, 4:])


def test_refused_parameters():
    for p in (tr.params(flags=4), tr.params(1048577), tr.params(plane_tolerance=-1.0), tr.params(plane_tolerance=float("inf")),
              tr.params(plane_tolerance=float("nan")), tr.params(normal_min=1.5), tr.params(normal_min=-0.1), tr.params(normal_min=float("nan"))):
        with pytest.raises(ValueError):
            tr.accumulate(np.zeros((2, 2, 4), np.float32), hit_guides(2, 2), tr.tr_camera(), None, p)
    tr.accumulate(np.zeros((2, 2, 4), np.float32), hit_guides(2, 2), tr.tr_camera(), None, tr.params(1048576, 0.5, 1.0, 3))


# ------------------------------------------------------------------------------------------------ reprojection geometry

@pytest.fixture(scope="module")
def cornell_path(P, pto):
    """The generator's Cornell at 96 x 72 under the quality experiment's camera path: per frame the camera and the §8.1 guides."""
    w, h = 96, 72
    sd = P.make_scene(P.native.PT_SCENE_CORNELL, 0, 3, w, h)
    cams = tc.camera_path(sd.cam)
    return w, h, sd, cams, [dc.guides(pto, pto.Scene(tc.with_camera(sd, c)), w, h) for c in cams]


def test_reprojection_agrees_with_float64(P, pto, cornell_path):
    """The checker's (fx, fy) against a float64 reprojection of the same world positions: within 1e-3 pixel on every valid pixel; and from
    frame 2 on at least 95 % of the hit pixels take history."""
    w, h, sd, cams, guides = cornell_path
    rng = np.random.default_rng(5)
    hist = None
    for k, (cam, g) in enumerate(zip(cams, guides)):
        res = tr.accumulate(rng.uniform(0, 1, (h, w, 4)).astype(np.float32), g, cam, hist, want_reproj=True)
        hits = g[..., 7].view(np.uint32) != tr.MISS
        if hist is not None:
            fx, fy, front = tc.reproject64(hist.cam, tc.world_positions64(pto, cam, g))
            valid = res.reproj[..., 2] == 1.0
            inside = hits & front & (fx >= -1.0) & (fx < w) & (fy >= -1.0) & (fy < h)
            edge = np.minimum(np.minimum(np.abs(fx + 1.0), np.abs(fx - w)), np.minimum(np.abs(fy + 1.0), np.abs(fy - h))) < 1e-3
            assert ((valid == inside) | edge).all()  # (the two may differ only where the float64 position is within the bound of the range's edge)
            assert valid.sum() > 0.9 * hits.sum()
            err = np.maximum(np.abs(res.reproj[..., 0] - fx), np.abs(res.reproj[..., 1] - fy))[valid]
            assert err.max() <= 1e-3, (k, err.max())
            took = (res.length > 1)[hits].mean()
            assert took >= 0.95, (k, took)
            assert res.taken == int((res.length > 1).sum())
        hist = res.history


@pytest.mark.parametrize("name", cs.TEMPORAL_CASES)
def test_reprojection_agrees_with_float64_under_general_cameras(P, pto, name):
    """The same check with an old camera that is rolled, skewed, anisotropic, off-centre, left-handed or mirrored (camera_space.cases)
    and a new one moved from it by move_camera: §9 inverts the old camera with the dual basis A, B, Cx and a sign test on det and den,
    which an orthogonal right-handed basis never exercises; reproject64 solves the 3 x 3 system. The tolerance is the 1e-3 pixel of
    the check above: fx = (sx + cx) / scale - 0.5 is rounded to 2^-24 of |sx / scale| + |cx / scale|, a few hundred pixels at most here
    (off_centre: the principal point 0.3 w and 0.9 h outside the image), so nothing of it has to be re-derived. Measured: at most 1.4e-5 pixel (off_centre)."""
    w, h = cs.W, cs.H
    sd = P.make_scene(P.native.PT_SCENE_CORNELL, 0, 3, w, h)
    old, new = cs.camera_pair(P, sd, name)
    g_old, g = (dc.guides(pto, pto.Scene(s), w, h) for s in (old, new))
    rng = np.random.default_rng(5)
    first = tr.accumulate(rng.uniform(0, 1, (h, w, 4)).astype(np.float32), g_old, old.cam)
    res = tr.accumulate(rng.uniform(0, 1, (h, w, 4)).astype(np.float32), g, new.cam, first.history, want_reproj=True)
    hits = g[..., 7].view(np.uint32) != tr.MISS
    fx, fy, front = tc.reproject64(first.history.cam, tc.world_positions64(pto, new.cam, g))
    valid = res.reproj[..., 2] == 1.0
    inside = hits & front & (fx >= -1.0) & (fx < w) & (fy >= -1.0) & (fy < h)
    edge = np.minimum(np.minimum(np.abs(fx + 1.0), np.abs(fx - w)), np.minimum(np.abs(fy + 1.0), np.abs(fy - h))) < 1e-3
    assert ((valid == inside) | edge).all()
    assert valid.sum() > 0.9 * hits.sum()
    err = np.maximum(np.abs(res.reproj[..., 0] - fx), np.abs(res.reproj[..., 1] - fy))[valid]
    print(f"reprojection under {name}: max error {err.max():.2e} pixel, {valid.sum()} of {hits.sum()} hit pixels valid, "
          f"took {(res.length > 1)[hits].mean():.3f}")
    assert err.max() <= 1e-3, (name, err.max())
    assert res.taken == int((res.length > 1).sum())


# ------------------------------------------------------------------------------------------------ exactness

def wall_colour(Pw):
    """Linear in world position."""
    c = np.ones(Pw.shape[:2] + (4,))
    c[..., 0] = 0.5 + 0.1 * Pw[..., 0]
    c[..., 1] = 0.4 + 0.08 * Pw[..., 1]
    c[..., 2] = 0.6 + 0.05 * Pw[..., 0] - 0.07 * Pw[..., 1]
    return c.astype(np.float32)


def check_affine_wall(P, pto, variant):
    """A fronto-parallel wall, the camera translated parallel to it by (1.4, 0.568) pixels, the colour linear in world position: the
    pixel -> world map is affine, so the bilinear history reproduces the new frame."""
    w, h = 64, 48
    cam0 = tc.axis_camera(P, w, h)
    cam1 = tc.move_camera(cam0, offset=(0.175, 0.071, 0.0))
    sd = tc.wall_and_quad(P, w, h, quad_x=50.0)  # (the quad is out of sight)
    g0, g1 = (dc.guides(pto, pto.Scene(tc.with_camera(sd, c)), w, h) for c in (cam0, cam1))
    c0, c1 = wall_colour(tc.world_positions64(pto, cam0, g0)), wall_colour(tc.world_positions64(pto, cam1, g1))
    res = tr.accumulate(c1, g1, cam1, tr.accumulate(c0, g0, cam0).history, variant=variant, want_reproj=True)
    fx, fy, valid = tr.accumulate(c1, g1, cam1, tr.accumulate(c0, g0, cam0).history, want_reproj=True).reproj.transpose(2, 0, 1)
    frac = (fx - np.floor(fx))[valid == 1.0]
    assert 0.3 < frac.min() and frac.max() < 0.5  # a non-integer shift
    four = (valid == 1.0) & (np.floor(fx) >= 0) & (np.floor(fx) + 1 <= w - 1) & (np.floor(fy) >= 0) & (np.floor(fy) + 1 <= h - 1)
    assert four.sum() > 0.9 * w * h
    assert (res.length[four] == 2).all()
    err = np.abs(res.image[..., :3] - c1[..., :3])[four].max()
    assert err <= 1e-4 * np.abs(c1[..., :3]).max(), err


def test_bilinear_history_reproduces_an_affine_frame(P, pto):
    check_affine_wall(P, pto, tr.SPEC)


@pytest.mark.parametrize("variant", [tr.NO_REPROJECTION, tr.NEAREST_TAP])
def test_affine_frame_catches_wrong_variants(P, pto, variant):
    with pytest.raises(AssertionError):
        check_affine_wall(P, pto, variant)


# ------------------------------------------------------------------------------------------------ disocclusion

def is_quad(g):
    ids = g[..., 7].view(np.uint32)
    return (ids == 2) | (ids == 3)


def check_moved_quad(P, pto, variant):
    """Still camera; the quad in front of the wall moves sideways by more than its width. A pixel that shows the quad in exactly one of
    the two frames starts again (l == 1, out == c bit for bit); a pixel that shows the wall in both has l == 2 and the mean of the two."""
    w, h = 64, 48
    cam = tc.axis_camera(P, w, h)
    g0, g1 = (dc.guides(pto, pto.Scene(tc.wall_and_quad(P, w, h, x)), w, h) for x in (-1.0, 0.2))
    q0, q1 = is_quad(g0), is_quad(g1)
    assert q0.sum() > 50 and q1.sum() > 50 and not (q0 & q1).any()
    a, b = random_frames(2, h, w, 6)
    res = tr.accumulate(b, g1, cam, tr.accumulate(a, g0, cam).history, variant=variant)
    one = q0 ^ q1
    assert (res.length[one] == 1).all() and same_bits(res.image[one], b[one])
    assert (res.length[~q0 & ~q1] == 2).all()
    mean = (a[..., :3].astype(np.float64) + b[..., :3]) / 2
    assert np.abs(res.image[..., :3] - mean)[~q0 & ~q1].max() <= 1e-6 * 4.0


def check_moved_camera(P, pto, variant):
    """The same scene with the camera moved sideways by 1.5 instead of the quad: a pixel all of whose four old taps show the other surface
    (wall uncovered by the quad's parallax, or the reverse) starts again; one whose four taps show its own surface has l == 2."""
    w, h = 64, 48
    cam0 = tc.axis_camera(P, w, h)
    cam1 = tc.move_camera(cam0, offset=(1.5, 0.0, 0.0))
    sd = tc.wall_and_quad(P, w, h)
    g0, g1 = (dc.guides(pto, pto.Scene(tc.with_camera(sd, c)), w, h) for c in (cam0, cam1))
    q0, q1 = is_quad(g0), is_quad(g1)
    fx, fy, _ = tc.reproject64(cam0, tc.world_positions64(pto, cam1, g1))
    x0, y0 = np.floor(fx).astype(int), np.floor(fy).astype(int)
    four = (x0 >= 0) & (x0 + 1 <= w - 1) & (y0 >= 0) & (y0 + 1 <= h - 1)
    xs, ys = np.clip(x0, 0, w - 2), np.clip(y0, 0, h - 2)
    taps = np.stack([q0[ys + j, xs + i] for j in (0, 1) for i in (0, 1)])
    other = four & (taps != q1[None]).all(axis=0)
    own = four & (taps == q1[None]).all(axis=0)
    assert (other & ~q1).sum() >= 20 and own.sum() > 0.5 * w * h and (own & q1).sum() > 20  # wall uncovered; quad seen in both
    a, b = random_frames(2, h, w, 7)
    res = tr.accumulate(b, g1, cam1, tr.accumulate(a, g0, cam0).history, variant=variant)
    assert (res.length[other] == 1).all() and same_bits(res.image[other], b[other])
    assert (res.length[own] == 2).all()


def test_disocclusion_by_a_moved_quad(P, pto):
    check_moved_quad(P, pto, tr.SPEC)


def test_disocclusion_by_a_moved_camera(P, pto):
    check_moved_camera(P, pto, tr.SPEC)


@pytest.mark.parametrize("variant", [tr.NO_PLANE_TEST, tr.FIXED_ALPHA])
def test_moved_quad_catches_wrong_variants(P, pto, variant):
    with pytest.raises(AssertionError):
        check_moved_quad(P, pto, variant)


def test_moved_camera_catches_a_missing_plane_test(P, pto):
    with pytest.raises(AssertionError):
        check_moved_camera(P, pto, tr.NO_PLANE_TEST)


# ------------------------------------------------------------------------------------------------ quality

# displayed RMSE of temporal + filter over that of the filter alone on the last frame, as the checker measures it; the bound
# of the test is the midpoint between this ratio and 1
MEASURED_RATIO = {"C1": 0.594, "C4": 0.597}


def quality_ratio(P, pto, kind, w=96, h=72, frames=8, ref_spp=2048):
    """The experiment of DESIGN.md §12 on the oracle's frames: 1 spp per frame with its own seed along the camera path, the default
    §8.2 filter over the last frame alone and over the accumulated image; errors against a ref_spp frame at the last camera."""
    sd = P.make_scene(kind, 0, 3, w, h)
    cams = tc.camera_path(sd.cam, frames)
    hist = None
    for k, cam in enumerate(cams):
        scene = pto.Scene(tc.with_camera(sd, cam))
        frame, _ = pto.render(scene, P.make_params(w, h, spp=1, max_depth=8, seed=1000 + k))
        g = dc.guides(pto, scene, w, h)
        res = tr.accumulate(frame, g, cam, hist)
        hist = res.history
    ref, _ = pto.render(scene, P.make_params(w, h, spp=ref_spp, max_depth=8, seed=99, streams=8))
    alone, both = dc.filter(frame, g), dc.filter(res.image, g)
    return {"display": (tc.display_rmse(alone, ref), tc.display_rmse(both, ref)),
            "linear": (tc.linear_rmse(alone, ref), tc.linear_rmse(both, ref)), "took": float((res.length > 1).mean())}


@pytest.mark.parametrize("name", ["C1", "C4"])
def test_quality(P, pto, name):
    kind = {"C1": P.native.PT_SCENE_CORNELL, "C4": P.native.PT_SCENE_CORNELL_GLASS}[name]
    q = quality_ratio(P, pto, kind)
    alone, both = q["display"]
    print(name, q)
    assert both < alone
    assert both / alone <= (MEASURED_RATIO[name] + 1.0) / 2.0, (both, alone)


# ------------------------------------------------------------------------------------------------ plumbing

def test_params_struct(P):
    N = P.native
    assert C.sizeof(N.pt_temporal_params) == 32 == C.sizeof(tr.tr_params)
    assert [f[0] for f in N.pt_temporal_params._fields_] == [f[0] for f in tr.tr_params._fields_]
    assert (N.PT_TEMPORAL_RESET, N.PT_TEMPORAL_MATCH_IDS) == (tr.RESET, tr.MATCH_IDS) == (1, 2)


def test_argument_checks_without_a_device(P):
    """tp's checks come first, then pt_denoise's checks of dp, then the NULL context."""
    N, lib = P.native, P.native.lib

    def err():
        return lib.pt_last_error(None).decode()

    tp, dp = N.pt_temporal_params(), N.pt_denoise_params()
    assert lib.pt_denoise_temporal(None, None, None, None, None) == N.PT_ERR_INVALID_ARGUMENT and "tp is NULL" in err()
    assert lib.pt_denoise_temporal(None, None, C.byref(tp), None, None) == N.PT_ERR_INVALID_ARGUMENT and "NULL context" in err()
    assert lib.pt_denoise_temporal(None, None, C.byref(tp), C.byref(dp), None) == N.PT_ERR_INVALID_ARGUMENT and "NULL context" in err()
    for field, value, what in (("flags", 4, "flag"), ("max_history", 1048577, "max_history"), ("plane_tolerance", -1.0, "plane_tolerance"),
                               ("plane_tolerance", float("nan"), "plane_tolerance"), ("plane_tolerance", float("inf"), "plane_tolerance"),
                               ("normal_min", 1.25, "normal_min"), ("normal_min", -0.5, "normal_min"), ("normal_min", float("nan"), "normal_min")):
        bad = N.pt_temporal_params()
        setattr(bad, field, value)
        bad_dp = N.pt_denoise_params(9)  # tp is checked before dp
        assert lib.pt_denoise_temporal(None, None, C.byref(bad), C.byref(bad_dp), None) == N.PT_ERR_INVALID_ARGUMENT and what in err(), (field, err())
    for field, value, what in (("flags", 4, "flag"), ("iterations", 9, "iterations"), ("sigma_color", -1.0, "sigma_color")):
        bad_dp = N.pt_denoise_params()
        setattr(bad_dp, field, value)
        assert lib.pt_denoise_temporal(None, None, C.byref(tp), C.byref(bad_dp), None) == N.PT_ERR_INVALID_ARGUMENT and what in err(), (field, err())
    ok = N.pt_temporal_params(1048576, 0.5, 1.0, N.PT_TEMPORAL_RESET | N.PT_TEMPORAL_MATCH_IDS)
    assert lib.pt_denoise_temporal(None, None, C.byref(ok), None, None) == N.PT_ERR_INVALID_ARGUMENT and "NULL context" in err()
    buf = np.zeros(8, np.float32)
    ptr, n = C.c_void_p(), C.c_uint64()
    assert lib.pt_temporal_read(None, buf.ctypes.data, 8) == N.PT_ERR_INVALID_ARGUMENT
    assert lib.pt_temporal_history_read(None, buf.ctypes.data, 8) == N.PT_ERR_INVALID_ARGUMENT
    assert lib.pt_temporal_device_ptr(None, C.byref(ptr), C.byref(n)) == N.PT_ERR_INVALID_ARGUMENT
