"""-m gpu: pt_denoise_temporal with PT_TEMPORAL_MOTION (docs/SPEC.md §9.1) on the device against the scalar checker of tests/motion_ref/.

The accumulated image, the history lengths, the guides, the filtered image, stats.paths and stats.reserved[0] are compared bit for bit
after every call of a sequence in which an object of triangles is translated and rotated, the camera moves, spheres move and change
radius, nothing moves, an unflagged call and a commit drop the snapshot; over frame sizes from 1x1 to 257x63, BVH2, BVH4Q and an LBVH
commit (blob order differs from id order). Also: updates from a device array, a static scene against the unflagged calls, the effect
(history that follows an object), refusals that change nothing, and the quality the flag buys on a moving object."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import denoise_checker as dc
import motion_cases as mc
import motion_checker as mr
import temporal_cases as tc

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (7, 5), (65, 3), (64, 48), (257, 63)]


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def oracle_scene(pto, sd):
    s = pto.Scene(sd)
    if len(sd.tri_mat) > 64:
        s.build_own_bvh()  # (the closest hit is the same; brute force over hundreds of triangles is slow)
    return s


class Mirror:
    """The device and the checker side by side: the checker's history and snapshot are carried here, the device's in the context.
    `scene_key` stands for the scene object and its commit: commit() renews it as SetScene does on the device."""

    def __init__(self, P, pto, r):
        self.P, self.pto, self.r, self.hist, self.scene_key = P, pto, r, None, 0

    def commit(self, sd, bvh=0):
        self.r.SetScene(sd, bvh)
        self.scene_key += 1

    def step(self, sd, ctx, motion=True, reset=False, match_ids=False, filter=True, **dn):
        """One DenoiseTemporal of the renderer's current frame; everything it hands out equals the checker's bit for bit."""
        P, r = self.P, self.r
        h, w = r.Params.height, r.Params.width
        tp = mr.params(flags=(mr.RESET if reset else 0) | (mr.MATCH_IDS if match_ids else 0) | (mr.MOTION if motion else 0))
        g = dc.guides(self.pto, oracle_scene(self.pto, sd), w, h)
        want = mr.accumulate(r.ReadFramebuffer(), g, sd.cam, sd.verts, sd.spheres, self.hist, tp, scene_key=self.scene_key)
        st = r.DenoiseTemporal(0, 0.0, 0.0, reset, match_ids, filter, motion=motion, **dn)
        img, length = r.ReadTemporal(), r.ReadHistoryLength()
        bad = np.argwhere((img.view(np.uint32) != want.image.view(np.uint32)).any(axis=2))
        assert len(bad) == 0, (ctx, len(bad), bad[:3].tolist(), img[tuple(bad[0])].tolist(), want.image[tuple(bad[0])].tolist())
        bad = np.argwhere(length.view(np.uint32) != want.length.view(np.uint32))
        assert len(bad) == 0, (ctx, len(bad), bad[:3].tolist(), length[tuple(bad[0])], want.length[tuple(bad[0])])
        assert st.paths == want.taken == int((length > 1).sum()) and st.rays == w * h, (ctx, st.paths, want.taken)
        assert st.reserved[0] == want.moved, (ctx, st.reserved[0], want.moved)
        assert same_bits(r.ReadGuides(), g), ctx
        if filter:
            assert same_bits(r.ReadDenoised(), dc.filter(want.image, g, dc.params(dn.get("iterations", 0)))), ctx
        self.hist = want.history
        return st, want


def frame(P, r, w, h, seed):
    r.Params = P.make_params(w, h, spp=1, max_depth=6, seed=seed)
    r.Render(0.0)


def moved_spheres(sd):
    s = sd.spheres.copy()
    s[:, 0] += 0.05
    s[1, 2] += 0.08
    s[0, 3] = 0.4  # one radius changes
    return dataclasses.replace(sd, spheres=s)


def the_sequence(P, pto, r, sd, w, h, bvh, as_device_array=None, **kw):
    """The sequence of the module's docstring. Each frame 1 spp with its own seed. as_device_array: how to hand vertices to
    UpdateGeometry (None: host memory)."""
    dev = as_device_array or (lambda v: v)
    m = Mirror(P, pto, r)
    m.commit(sd, bvh)
    big = w * h > 1000
    frame(P, r, w, h, 11)
    st, want = m.step(sd, "first", reset=True, **kw)
    assert st.paths == 0 and st.reserved[0] == 0 and not want.used_snapshot
    sd = mc.move_object(sd, (0.0, 0.0, 0.15))
    r.UpdateGeometry(verts=dev(sd.verts))
    frame(P, r, w, h, 12)
    st, want = m.step(sd, "object towards the camera", **kw)
    assert want.used_snapshot
    if big:  # the object's pixels all count as moved, and its interior keeps its history
        obj = mc.object_mask(want.history.g8, sd)
        assert st.reserved[0] == obj.sum() > 20 and (want.length[obj] == 2).mean() > 0.4
    cam = tc.move_camera(sd.cam, 0.03, yaw_deg=0.7, offset=(0.0, 0.01, 0.0))
    sd = tc.with_camera(mc.move_object(sd, (0.05, 0.02, 0.05)), cam)
    r.SetCamera(cam)
    r.UpdateGeometry(verts=dev(sd.verts))
    frame(P, r, w, h, 13)
    st, want = m.step(sd, "camera and object", **kw)
    sd = mc.move_object(sd, yaw_deg=25.0)
    r.UpdateGeometry(verts=dev(sd.verts))
    frame(P, r, w, h, 14)
    st, want = m.step(sd, "object rotated", **kw)
    if big:
        assert st.reserved[0] > 20
    sd = moved_spheres(sd)
    r.UpdateGeometry(spheres=sd.spheres)
    frame(P, r, w, h, 15)
    st, want = m.step(sd, "spheres moved, one radius changed", **kw)
    if big:
        ids = want.history.g8[..., 7].view(np.uint32)
        assert st.reserved[0] == ((ids >= len(sd.tri_mat)) & (ids != mr.MISS)).sum() > 20
    frame(P, r, w, h, 16)
    st, want = m.step(sd, "nothing moved", **kw)
    assert st.reserved[0] == 0 and want.used_snapshot
    frame(P, r, w, h, 17)
    st, want = m.step(sd, "unflagged", motion=False, **kw)
    assert not want.history.has_snapshot
    sd = mc.move_object(sd, (0.0, 0.0, -0.1))
    r.UpdateGeometry(verts=dev(sd.verts))
    frame(P, r, w, h, 18)
    st, want = m.step(sd, "flagged after unflagged: plain §9", **kw)
    assert st.reserved[0] == 0 and not want.used_snapshot
    sd = mc.move_object(sd, (0.0, 0.0, 0.1))
    m.commit(sd, bvh)
    frame(P, r, w, h, 19)
    st, want = m.step(sd, "flagged after a commit: plain §9", **kw)
    assert st.reserved[0] == 0 and not want.used_snapshot
    sd = mc.move_object(sd, (-0.05, 0.0, 0.1))
    r.UpdateGeometry(verts=dev(sd.verts))
    frame(P, r, w, h, 20)
    st, want = m.step(sd, "moved again", **kw)
    assert want.used_snapshot and (not big or st.reserved[0] > 20)
    return m, sd


def cornell(P, w, h):
    return mc.with_object(P, P.make_scene(P.native.PT_SCENE_CORNELL, 0, 3, w, h))


def cornell_tess(P, w, h):
    sd = mc.with_object(P, P.make_scene(P.native.PT_SCENE_CORNELL_TESS, 300, 3, w, h))
    assert len(sd.tri_mat) > 192  # BVH4Q by default
    return sd


@pytest.mark.parametrize("w,h", SHAPES)
def test_sequence_cornell(P, pto, renderer, w, h):
    the_sequence(P, pto, renderer, cornell(P, w, h), w, h, 0, iterations=2)
    assert renderer.BvhInfo().width == P.native.PT_BVH_WIDTH_2


@pytest.mark.parametrize("w,h", [(7, 5), (257, 63)])
def test_sequence_tessellated_bvh4q(P, pto, renderer, w, h):
    the_sequence(P, pto, renderer, cornell_tess(P, w, h), w, h, 0, filter=False)
    assert renderer.BvhInfo().width == P.native.PT_BVH_WIDTH_4Q


@pytest.mark.parametrize("tess", [False, True])
def test_sequence_lbvh_commit(P, pto, renderer, tess):
    """After a PT_BVH_BUILD_LBVH commit the blob order differs from the id order: what d_blob_of is for."""
    N = P.native
    w, h = 64, 48
    sd = cornell_tess(P, w, h) if tess else cornell(P, w, h)
    the_sequence(P, pto, renderer, sd, w, h, N.PT_BVH_WIDTH_4Q | N.PT_BVH_BUILD_LBVH, filter=False, match_ids=tess)


def test_updates_from_a_device_array(P, pto, renderer):
    torch = pytest.importorskip("torch")
    w, h = 64, 48
    the_sequence(P, pto, renderer, cornell(P, w, h), w, h, 0, filter=False,
                 as_device_array=lambda v: torch.as_tensor(np.ascontiguousarray(v, np.float32), device="cuda"))


def test_static_scene_equals_the_unflagged_calls(P, renderer):
    """A flagged sequence on a scene that never moves (the camera does) equals the unflagged sequence bit for bit: in the first half no
    update runs between the calls, in the second an update to the same vertices does, so every pixel goes through the motion pass and
    counts as unmoved."""
    w, h = 64, 48
    sd = cornell(P, w, h)
    got = {}
    for motion in (False, True):
        renderer.SetScene(sd, 0)
        out = []
        for k, cam in enumerate(tc.camera_path(sd.cam, 6)):
            renderer.SetCamera(cam)
            if k >= 3:
                renderer.UpdateGeometry(verts=sd.verts, spheres=sd.spheres)
            frame(P, renderer, w, h, 30 + k)
            st = renderer.DenoiseTemporal(reset=k == 0, motion=motion)
            assert st.reserved[0] == 0
            out.append((renderer.ReadTemporal(), renderer.ReadHistoryLength(), renderer.ReadDenoised(), st.paths))
        got[motion] = out
    for (a, la, da, pa), (b, lb, db, pb) in zip(got[False], got[True]):
        assert same_bits(a, b) and same_bits(la, lb) and same_bits(da, db) and pa == pb
    assert got[True][-1][3] > 0.5 * w * h


def test_history_follows_the_object(P, renderer):
    """tests/test_temporal_motion.py's quad that comes 0.1 closer per call, on the device: l = k inside it with the flag (within 1e-6 k,
    the bound derived there), l = 1 without."""
    w, h = 96, 72
    cam = tc.axis_camera(P, w, h)

    def quad_at(k):
        sd = tc.wall_and_quad(P, w, h, quad_x=-0.4, cam=cam)
        v = sd.verts.copy()
        v[2:4, 2::3] = -2.0 + 0.1 * k
        return dataclasses.replace(sd, verts=v)

    for motion in (True, False):
        renderer.SetScene(quad_at(0), 0)
        for k in range(1, 5):
            if k > 1:
                renderer.UpdateGeometry(verts=quad_at(k - 1).verts)
            frame(P, renderer, w, h, 40 + k)
            st = renderer.DenoiseTemporal(max_history=64, reset=k == 1, filter=False, motion=motion)
            ids = renderer.ReadGuides()[..., 7].view(np.uint32)
            quad = (ids == 2) | (ids == 3)
            inside = mc.interior(quad)
            length = renderer.ReadHistoryLength()
            assert inside.sum() > 100
            if motion:
                assert np.abs(length[inside] - k).max() <= 1e-6 * k, (k, length[inside].min(), length[inside].max())
                assert st.reserved[0] == (quad.sum() if k > 1 else 0)
            else:
                assert (length[inside] == 1).all() and st.reserved[0] == 0


def test_refusals_change_nothing(P, pto, renderer):
    """A refused call (bad tp, bad dp, a detached scene, an unknown bit beside the flag) leaves image, lengths, history and snapshot as
    they were: the next flagged call equals the checker run with the untouched history and snapshot."""
    N, lib = P.native, P.native.lib
    w, h = 64, 48
    sd = cornell(P, w, h)
    m = Mirror(P, pto, renderer)
    m.commit(sd)
    frame(P, renderer, w, h, 51)
    m.step(sd, "first", reset=True)
    sd = mc.move_object(sd, (0.0, 0.0, 0.15))
    renderer.UpdateGeometry(verts=sd.verts)
    frame(P, renderer, w, h, 52)
    st, _ = m.step(sd, "second")
    assert st.reserved[0] > 20
    kept = [renderer.ReadTemporal(), renderer.ReadHistoryLength(), renderer.ReadDenoised(), renderer.ReadGuides()]
    ctx, scene = renderer._ctx, renderer._scene
    dp = N.pt_denoise_params()
    M = N.PT_TEMPORAL_MOTION
    for tp, d in ((N.pt_temporal_params(1048577, 0, 0, M), dp), (N.pt_temporal_params(0, -1.0, 0, M), dp), (N.pt_temporal_params(0, 0, 0, M | 4), dp),
                  (N.pt_temporal_params(0, 0, 0, M | 16), dp), (N.pt_temporal_params(0, 0, 0, 4), dp), (N.pt_temporal_params(0, 0, 0, M), N.pt_denoise_params(9)),
                  (N.pt_temporal_params(0, 0, 0, M), N.pt_denoise_params(0, 0, 0, 0, 0, 8))):
        assert lib.pt_denoise_temporal(ctx, scene, C.byref(tp), C.byref(d), None) == N.PT_ERR_INVALID_ARGUMENT
    det = C.c_void_p()
    assert lib.pt_scene_create(None, C.byref(det)) == 0
    try:
        assert lib.pt_denoise_temporal(ctx, det, C.byref(N.pt_temporal_params(0, 0, 0, M)), C.byref(dp), None) == N.PT_ERR_UNSUPPORTED
    finally:
        lib.pt_scene_destroy(det)
    now = [renderer.ReadTemporal(), renderer.ReadHistoryLength(), renderer.ReadDenoised(), renderer.ReadGuides()]
    assert all(same_bits(a, b) for a, b in zip(now, kept))
    sd = mc.move_object(sd, (0.04, 0.0, 0.1), yaw_deg=10.0)
    renderer.UpdateGeometry(verts=sd.verts)
    frame(P, renderer, w, h, 53)
    st, want = m.step(sd, "after the refusals")
    assert want.used_snapshot and st.reserved[0] > 20 and want.length.max() == 3


# displayed RMSE of the filtered image over the moved object's pixels, flagged over unflagged, as measured on the device (0.1049 ->
# 0.0846); the bound of the test is the midpoint between this ratio and 1
MEASURED_RATIO = 0.807


def test_quality(P, renderer):
    """Eight 1-spp frames of Cornell with the object coming closer under a still camera, at 320 x 240, against a 4096-spp frame of the
    last geometry."""
    q = mc.device_quality(P, renderer, 320, 240)
    plain, flagged = q["display"]
    print("motion quality", q, flagged / plain)
    assert q["pixels"] > 1000 and q["moved"] == q["pixels"]
    assert flagged < plain
    assert flagged / plain <= (MEASURED_RATIO + 1.0) / 2.0, (flagged, plain)
