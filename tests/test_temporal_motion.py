"""PT_TEMPORAL_MOTION (docs/SPEC.md §9.1) without a GPU: the scalar checker of tests/motion_ref/ against tests/temporal_ref/ where nothing
moves, against float64 numpy where something does — history that follows an object, an affine frame reproduced under in-plane sliding,
the reprojection coordinates of moved triangles and spheres, disocclusion — each wrong variant of the checker shown to break one of
them, and the API's plumbing.

The device is held to the checker bit for bit by tests/test_gpu_temporal_motion.py."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import denoise_checker as dc
import motion_cases as mc
import motion_checker as mr
import temporal_cases as tc
import temporal_checker as tr


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def random_frames(n, h, w, seed):
    rng = np.random.default_rng(seed)
    return [rng.uniform(0.0, 4.0, (h, w, 4)).astype(np.float32) for _ in range(n)]


def guides(pto, sd, w, h):
    return dc.guides(pto, pto.Scene(sd), w, h)


def as_tr(hist):
    """The §9 part of a motion History, for tests/temporal_checker.py."""
    return None if hist is None else tr.History(hist.g8, hist.h, tr.camera(hist.cam))


def flagged(**kw):
    return mr.params(flags=mr.MOTION, **kw)


def ids_of(g):
    return g[..., 7].view(np.uint32)


interior = mc.interior


def with_quad_z(sd, z):
    v = sd.verts.copy()
    v[2:4, 2::3] = z
    return dataclasses.replace(sd, verts=v)


# ------------------------------------------------------------------------------------------------ 1. nothing moved: §9 exactly

def test_static_scene_equals_section_9(P, pto):
    """Cornell under the quality experiment's camera path, four flagged calls: image, lengths and taken equal tests/temporal_ref/'s bit
    for bit, no pixel counts as moved, and from the second call on the snapshot is in use."""
    w, h = 48, 36
    sd = P.make_scene(P.native.PT_SCENE_CORNELL, 0, 3, w, h)
    hm, ht = None, None
    for k, (cam, c) in enumerate(zip(tc.camera_path(sd.cam, 4), random_frames(4, h, w, 1))):
        g = guides(pto, tc.with_camera(sd, cam), w, h)
        a = mr.accumulate(c, g, cam, sd.verts, sd.spheres, hm, flagged())
        b = tr.accumulate(c, g, cam, ht)
        assert same_bits(a.image, b.image) and same_bits(a.length, b.length) and a.taken == b.taken, k
        assert a.moved == 0 and a.used_snapshot == (k > 0)
        assert k == 0 or a.taken > 0.9 * (ids_of(g) != mr.MISS).sum() > 0.5 * w * h
        hm, ht = a.history, b.history


def test_unmoved_background_equals_section_9(P, pto):
    """One object moves in front of a wall under a moving camera: every pixel whose primitive did not move is §9's, from the same
    history, bit for bit."""
    w, h = 64, 48
    cams = [tc.move_camera(tc.axis_camera(P, w, h), offset=(0.05 * k, 0.02 * k, 0.0)) for k in range(4)]
    hm = None
    for k, (cam, c) in enumerate(zip(cams, random_frames(4, h, w, 2))):
        sd = with_quad_z(tc.wall_and_quad(P, w, h, cam=cam), -2.0 + 0.1 * k)
        g = guides(pto, sd, w, h)
        a = mr.accumulate(c, g, cam, sd.verts, sd.spheres, hm, flagged())
        b = tr.accumulate(c, g, cam, as_tr(hm))
        still = ~a.moved_mask
        assert same_bits(a.image[still], b.image[still]) and same_bits(a.length[still], b.length[still]), k
        if k:
            quad = ids_of(g) >= 2
            assert a.moved == quad.sum() > 50 and (a.moved_mask == quad).all()
            assert (a.length[still] > 1).mean() > 0.9
        hm = a.history


# ------------------------------------------------------------------------------------------------ 2. history follows the object

def check_history_follows(P, pto, variant):
    """A quad facing a still camera comes 0.1 closer per call from distance 2 (tau_p times the distance is 0.016). With the flag its
    interior pixels have l = k after call k — within 1e-6 k: sw, sl, 1/sw, their product and the sum are at most 8 roundings of 2^-24
    each —; without it they start again at every call."""
    w, h = 96, 72
    cam = tc.axis_camera(P, w, h)
    hm = ht = None
    for k, c in enumerate(random_frames(4, h, w, 3), 1):
        sd = with_quad_z(tc.wall_and_quad(P, w, h, quad_x=-0.4), -2.0 + 0.1 * (k - 1))
        g = guides(pto, sd, w, h)
        a = mr.accumulate(c, g, cam, sd.verts, sd.spheres, hm, flagged(max_history=64), variant=variant)
        b = tr.accumulate(c, g, cam, ht, tr.params(64))
        inside = interior(ids_of(g) >= 2)
        assert inside.sum() > 100
        assert np.abs(a.length[inside] - k).max() <= 1e-6 * k, (k, a.length[inside].min(), a.length[inside].max())
        assert (b.length[inside] == 1).all(), k
        wall = interior(ids_of(g) < 2)
        assert (a.length[wall] == k).all() and (b.length[wall] == k).all()
        hm, ht = a.history, b.history


def test_history_follows_the_object(P, pto):
    check_history_follows(P, pto, mr.SPEC)


# ------------------------------------------------------------------------------------------------ 3. in-plane sliding

def own_colour(Pw, quad, x_left):
    """Linear in the surface's own coordinates: the wall's are the world's, the quad's are relative to its left edge."""
    ox = np.where(quad, Pw[..., 0] - x_left, Pw[..., 0])
    c = np.ones(Pw.shape[:2] + (4,))
    c[..., 0] = 0.5 + 1.0 * ox
    c[..., 1] = 0.4 + 0.08 * Pw[..., 1]
    c[..., 2] = 0.6 + 0.5 * ox - 0.07 * Pw[..., 1]
    return c.astype(np.float32)


def slide(P, pto):
    """The quad slides by 0.02 (0.36 pixel) in its own plane under a still camera; the frames are an affine function of its own
    coordinates. Returns the second frame, the pixels whose four old taps lie well inside the quad, the flagged result, §9's."""
    w, h = 96, 72
    cam = tc.axis_camera(P, w, h)
    x0, x1 = -0.4, -0.38
    sd0, sd1 = tc.wall_and_quad(P, w, h, quad_x=x0), tc.wall_and_quad(P, w, h, quad_x=x1)
    g0, g1 = guides(pto, sd0, w, h), guides(pto, sd1, w, h)
    q0, q1 = ids_of(g0) >= 2, ids_of(g1) >= 2
    c0 = own_colour(tc.world_positions64(pto, cam, g0), q0, x0)
    c1 = own_colour(tc.world_positions64(pto, cam, g1), q1, x1)
    first = mr.accumulate(c0, g0, cam, sd0.verts, sd0.spheres, None, flagged())
    a = mr.accumulate(c1, g1, cam, sd1.verts, sd1.spheres, first.history, flagged(), want_reproj=True)
    b = tr.accumulate(c1, g1, cam, as_tr(first.history))
    inside = interior(q0 & q1)
    assert inside.sum() > 50 and a.moved == q1.sum()
    return c1, inside, a, b


def test_in_plane_sliding_reproduces_an_affine_frame(P, pto):
    c1, inside, a, b = slide(P, pto)
    fx = a.reproj[..., 0][inside]
    frac = fx - np.floor(fx)
    assert 0.6 < frac.min() and frac.max() < 0.7  # a sub-pixel slide: the old point lies 0.36 pixel to the left
    assert (a.length[inside] == 2).all()
    err = np.abs(a.image[..., :3] - c1[..., :3])[inside].max()
    assert err <= 1e-4 * np.abs(c1[..., :3]).max(), err  # (the bound of tests/test_temporal.py's affine wall)


def test_in_plane_sliding_without_the_flag_is_off_by_the_slide(P, pto):
    """§9's limitation, shown: the quad passes the plane and normal tests against its old self and keeps the colour of the wrong
    surface points — red has slope 1 per unit, the slide is 0.02 and the blend halves it."""
    c1, inside, a, b = slide(P, pto)
    assert (b.length[inside] == 2).all()
    off = np.abs(b.image[..., 0] - c1[..., 0])[inside]
    assert np.abs(off - 0.01).max() <= 1e-4


# ------------------------------------------------------------------------------------------------ 4. reprojection coordinates

def tri_and_sphere(P, w, h, cam, angle_deg=0.0, shift=(0.0, 0.0, 0.0), centre=(1.2, 0.3, -2.5), radius=0.5):
    """A large triangle facing +z, rotated about the y axis through its centroid and shifted; a sphere beside it."""
    v = np.array([[-2.0, -1.2, -3.0], [0.4, -1.2, -3.0], [-0.8, 1.4, -3.0]], np.float64)
    ctr = v.mean(axis=0)
    a = np.radians(angle_deg)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    v = (v - ctr) @ R.T + ctr + np.asarray(shift)
    sd = P.SceneData()
    sd.verts = v.reshape(1, 9).astype(np.float32)
    sd.tri_mat = np.array([0], np.uint32)
    sd.spheres = np.array([list(centre) + [radius]], np.float32)
    sd.sph_mat = np.array([1], np.uint32)
    sd.mats = np.zeros(2, P.MATERIAL_DTYPE)
    sd.mats["albedo"] = [(0.7, 0.7, 0.7), (0.8, 0.3, 0.2)]
    sd.cam = cam
    return sd


def moved_points64(sd0, sd1, Pw, ids):
    """float64: where the surface point under each pixel of the new scene sd1 was in the old scene sd0."""
    out = np.full(Pw.shape, np.nan)
    v1, v0 = sd1.verts.astype(np.float64).reshape(-1, 3, 3), sd0.verts.astype(np.float64).reshape(-1, 3, 3)
    tri = ids == 0
    E1 = np.stack([v1[0, 1] - v1[0, 0], v1[0, 2] - v1[0, 0]], axis=1)  # 3 x 2
    uv = np.linalg.lstsq(E1, (Pw[tri] - v1[0, 0]).T, rcond=None)[0].T
    out[tri] = v0[0, 0] + uv[:, :1] * (v0[0, 1] - v0[0, 0]) + uv[:, 1:] * (v0[0, 2] - v0[0, 0])
    sph = ids == 1
    s1, s0 = sd1.spheres.astype(np.float64)[0], sd0.spheres.astype(np.float64)[0]
    out[sph] = s0[:3] + (Pw[sph] - s1[:3]) * (s0[3] / s1[3])
    return out


def check_reprojection(P, pto, variant):
    """A triangle that turns by 35 degrees (cos = 0.82 < tau_n) and shifts, a sphere that shifts and grows, a camera that moves and
    yaws: (fx, fy) of every moved pixel within 1e-3 pixel of the float64 solve; the triangle's interior keeps its history although its
    normal turned past tau_n, because the taps are tested against the surface as it was."""
    w, h = 64, 48
    cam0 = tc.axis_camera(P, w, h)
    cam1 = tc.move_camera(cam0, 0.04, yaw_deg=0.8, offset=(0.0, 0.03, 0.02))
    sd0 = tri_and_sphere(P, w, h, cam0)
    sd1 = tri_and_sphere(P, w, h, cam1, 35.0, (0.1, -0.05, 0.2), (1.05, 0.35, -2.3), 0.6)
    g0, g1 = guides(pto, sd0, w, h), guides(pto, sd1, w, h)
    c0, c1 = random_frames(2, h, w, 4)
    first = mr.accumulate(c0, g0, cam0, sd0.verts, sd0.spheres, None, flagged())
    res = mr.accumulate(c1, g1, cam1, sd1.verts, sd1.spheres, first.history, flagged(), variant=variant, want_reproj=True)
    ids = ids_of(g1)
    assert (ids == 0).sum() > 200 and (ids == 1).sum() > 100 and res.moved == (ids != mr.MISS).sum()
    Pm = moved_points64(sd0, sd1, tc.world_positions64(pto, cam1, g1), ids)
    fx, fy, front = tc.reproject64(cam0, Pm)
    valid = res.reproj[..., 2] == 1.0
    well_inside = (ids != mr.MISS) & front & (fx >= -0.99) & (fx < w - 0.01) & (fy >= -0.99) & (fy < h - 0.01)
    assert valid[well_inside].all() and well_inside.sum() > 0.9 * (ids != mr.MISS).sum()
    for prim in (0, 1):
        m = valid & (ids == prim)
        err = np.maximum(np.abs(res.reproj[..., 0] - fx), np.abs(res.reproj[..., 1] - fy))[m]
        assert err.max() <= 1e-3, (prim, err.max())
    # the taps must land in the old image of the same primitive: judge the pixels whose old position lies well inside it
    x0, y0 = np.floor(np.nan_to_num(fx)).astype(int), np.floor(np.nan_to_num(fy)).astype(int)
    ok = well_inside & (x0 >= 0) & (x0 + 1 < w) & (y0 >= 0) & (y0 + 1 < h)
    old_tri = interior(ids_of(g0) == 0, 1)
    kept = ok & (ids == 0)
    kept[kept] = old_tri[y0[kept], x0[kept]]
    assert kept.sum() > 100 and (res.length[kept] == 2).all(), (kept.sum(), (res.length[kept] == 2).mean())


def test_reprojection_agrees_with_float64(P, pto):
    check_reprojection(P, pto, mr.SPEC)


# ------------------------------------------------------------------------------------------------ 5. disocclusion

def test_disocclusion_and_an_old_triangle_without_area(P, pto):
    """Still camera; the quad moves sideways by more than its width. The wall it uncovers starts again (l = 1, out = c bit for bit),
    the quad brings its history along (l = 2 inside), the wall seen in both frames has l = 2. Then the same call with a snapshot in
    which triangle 2 has no area: its pixels have no history and nothing is NaN."""
    w, h = 64, 48
    cam = tc.axis_camera(P, w, h)
    sd0, sd1 = tc.wall_and_quad(P, w, h, -1.0), tc.wall_and_quad(P, w, h, 0.2)
    g0, g1 = guides(pto, sd0, w, h), guides(pto, sd1, w, h)
    q0, q1 = ids_of(g0) >= 2, ids_of(g1) >= 2
    assert q0.sum() > 50 and q1.sum() > 50 and not (q0 & q1).any()
    a, b = random_frames(2, h, w, 5)
    first = mr.accumulate(a, g0, cam, sd0.verts, sd0.spheres, None, flagged())
    res = mr.accumulate(b, g1, cam, sd1.verts, sd1.spheres, first.history, flagged())
    assert (res.length[q0] == 1).all() and same_bits(res.image[q0], b[q0])
    assert (res.length[interior(q1)] == 2).all()
    assert (res.length[~q0 & ~q1] == 2).all()
    flat = first.history
    flat.snap_tris = flat.snap_tris.copy()
    flat.snap_tris[2, 3:6] = flat.snap_tris[2, 0:3]  # v1' = v0'
    res2 = mr.accumulate(b, g1, cam, sd1.verts, sd1.spheres, flat, flagged())
    t2 = ids_of(g1) == 2
    assert t2.sum() > 20 and (res2.length[t2] == 1).all() and same_bits(res2.image[t2], b[t2])
    assert np.isfinite(res2.image).all() and np.isfinite(res2.length).all()
    assert (res2.length[interior(ids_of(g1) == 3)] == 2).all()


# ------------------------------------------------------------------------------------------------ 6. negative controls

@pytest.mark.parametrize("variant", [mr.IGNORE_MOTION, mr.NEW_PLANE])
def test_history_follows_catches_wrong_variants(P, pto, variant):
    with pytest.raises(AssertionError):
        check_history_follows(P, pto, variant)


@pytest.mark.parametrize("variant", [mr.NEW_NORMAL, mr.NO_RADIUS_RATIO])
def test_reprojection_catches_wrong_variants(P, pto, variant):
    with pytest.raises(AssertionError):
        check_reprojection(P, pto, variant)


# ------------------------------------------------------------------------------------------------ 7. plumbing

def test_flag_values(P):
    N = P.native
    assert N.PT_TEMPORAL_MOTION == 8 == mr.MOTION
    assert C.sizeof(N.pt_temporal_params) == 32 == C.sizeof(mr.mr_params)
    for f in (4, 16):
        with pytest.raises(ValueError):
            mr.accumulate(np.zeros((2, 2, 4), np.float32), np.zeros((2, 2, 8), np.float32), mr.mr_camera(), np.zeros((0, 9)), np.zeros((0, 4)),
                          None, mr.params(flags=f))


def test_argument_checks_without_a_device(P):
    """The new bit passes tp's checks and the call ends at the NULL context; bit 4 stays unassigned."""
    N, lib = P.native, P.native.lib

    def err():
        return lib.pt_last_error(None).decode()

    for flags in (8, 8 | 3):
        tp = N.pt_temporal_params(0, 0.0, 0.0, flags)
        assert lib.pt_denoise_temporal(None, None, C.byref(tp), None, None) == N.PT_ERR_INVALID_ARGUMENT and "NULL context" in err()
    for flags in (4, 16, 8 | 4):
        tp = N.pt_temporal_params(0, 0.0, 0.0, flags)
        assert lib.pt_denoise_temporal(None, None, C.byref(tp), None, None) == N.PT_ERR_INVALID_ARGUMENT and "flag" in err()


# ------------------------------------------------------------------------------------------------ quality

# displayed RMSE over the moved object's pixels, flagged over unflagged, as the checkers measure it on the oracle's frames (DESIGN.md
# §12.1); the bound of the test is the midpoint between this ratio and 1
MEASURED_RATIO = 0.520


def test_quality(P, pto):
    """Eight 1-spp frames of Cornell with the object coming closer under a still camera, 96 x 72, against a 2048-spp frame of the last
    geometry."""
    q = mc.oracle_quality(P, pto, dc, mr)
    plain, with_flag = q["display"]
    print("motion quality", q, with_flag / plain)
    assert q["pixels"] > 400 and q["moved"] == q["pixels"]
    assert with_flag < plain
    assert with_flag / plain <= (MEASURED_RATIO + 1.0) / 2.0, (with_flag, plain)
