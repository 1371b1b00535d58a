"""-m gpu: pt_denoise_temporal (docs/SPEC.md §9) on the device against the scalar checker of tests/temporal_ref/.

The accumulated image, the history lengths, the guides, the filtered image and stats.paths are compared bit for bit after every call of
sequences in which the seed, the camera and the geometry change, over frame sizes from 1x1 to 257x63, scenes with triangles, spheres and
sky, both builders, with and without the filter, every flag and the history caps. Also: the equivalence with PT_FLAG_ACCUMULATE under a
still camera, what survives which call, every refusal, and the quality it buys on the Cornell boxes."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import denoise_checker as dc
import temporal_cases as tc
import temporal_checker as tr

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (7, 5), (65, 3), (64, 48), (257, 63)]


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def oracle_scene(pto, sd):
    s = pto.Scene(sd)
    if len(sd.tri_mat) > 64:
        s.build_own_bvh()  # (the closest hit is the same; brute force over a soup is slow)
    return s


class Mirror:
    """The device and the checker side by side: the checker's history is carried here, the device's in the context."""

    def __init__(self, P, pto, r):
        self.P, self.pto, self.r, self.hist = P, pto, r, None

    def expect(self, sd, tp):
        """What the checker makes of the renderer's current frame on `sd` with the history so far (nothing is committed)."""
        h, w = self.r.Params.height, self.r.Params.width
        g = dc.guides(self.pto, oracle_scene(self.pto, sd), w, h)
        return g, tr.accumulate(self.r.ReadFramebuffer(), g, sd.cam, self.hist, tp)

    def step(self, sd, ctx, max_history=0, plane_tolerance=0.0, normal_min=0.0, reset=False, match_ids=False, filter=True, **dn):
        """One DenoiseTemporal of the renderer's current frame; everything it hands out equals the checker's bit for bit."""
        P, r = self.P, self.r
        h, w = r.Params.height, r.Params.width
        tp = tr.params(max_history, plane_tolerance, normal_min, (tr.RESET if reset else 0) | (tr.MATCH_IDS if match_ids else 0))
        g, want = self.expect(sd, tp)
        st = r.DenoiseTemporal(max_history, plane_tolerance, normal_min, reset, match_ids, filter, **dn)
        img, length = r.ReadTemporal(), r.ReadHistoryLength()
        bad = np.argwhere((img.view(np.uint32) != want.image.view(np.uint32)).any(axis=2))
        assert len(bad) == 0, (ctx, len(bad), bad[:3].tolist(), img[tuple(bad[0])].tolist(), want.image[tuple(bad[0])].tolist())
        bad = np.argwhere(length.view(np.uint32) != want.length.view(np.uint32))
        assert len(bad) == 0, (ctx, len(bad), bad[:3].tolist(), length[tuple(bad[0])], want.length[tuple(bad[0])])
        assert st.paths == want.taken == int((length > 1).sum()) and st.rays == w * h, (ctx, st.paths, want.taken)
        assert same_bits(r.ReadGuides(), g), ctx
        if filter and not dn.get("guides_only"):
            dp = dc.params(dn.get("iterations", 0), dn.get("sigma_color", 0.0), dn.get("sigma_normal", 0.0), dn.get("sigma_depth", 0.0),
                           dn.get("sigma_albedo", 0.0), 0 if dn.get("edge_stops", True) else dc.NO_EDGE_STOPS)
            assert same_bits(r.ReadDenoised(), dc.filter(want.image, g, dp)), ctx
            assert st.iterations == (dn.get("iterations", 0) or dc.defaults()[0])
        else:
            with pytest.raises(P.PtException) as e:
                r.ReadDenoised()
            assert e.value.status == P.native.PT_ERR_NOT_COMMITTED and st.iterations == 0
        self.hist = want.history
        return st, want


def frame(P, r, w, h, seed, **kw):
    r.Params = P.make_params(w, h, spp=1, max_depth=6, seed=seed, **kw)
    r.Render(0.0)


def soup(P, w, h):
    """The triangle soup with its sky: pixels that miss, and history that lands on misses."""
    sd = P.make_scene(P.native.PT_SCENE_TRIANGLE_SOUP, 4000, 5, w, h)
    return dataclasses.replace(sd, sky=np.array([0.3, 0.4, 0.6], np.float32))


def moved_verts(sd):
    v = sd.verts.copy().reshape(-1, 3, 3)
    v[:, :, 0] += 0.06 * np.sin(np.arange(len(v)))[:, None]
    v[:, :, 2] -= 0.04
    return v.reshape(-1, 9)


def five_calls(P, pto, r, sd, w, h, bvh, **kw):
    """First frame; same camera, new seed; camera translated; camera yawed; triangles moved. Each frame 1 spp with its own seed."""
    r.SetScene(sd, bvh)
    m = Mirror(P, pto, r)
    frame(P, r, w, h, 11)
    st, _ = m.step(sd, "first", reset=True, **kw)
    assert st.paths == 0
    frame(P, r, w, h, 12)
    st, want = m.step(sd, "new seed", **kw)
    hits = want.history.g8[..., 7].view(np.uint32) != tr.MISS
    assert st.paths == (0 if kw.get("max_history") == 1 else hits.sum())  # a still camera: every hit pixel accumulates, no miss does
    cam = tc.move_camera(sd.cam, 0.03, offset=(0.0, 0.01, 0.0))
    sd = tc.with_camera(sd, cam)
    r.SetCamera(cam)
    frame(P, r, w, h, 13)
    m.step(sd, "translated", **kw)
    cam = tc.move_camera(cam, yaw_deg=1.5)
    sd = tc.with_camera(sd, cam)
    r.SetCamera(cam)
    frame(P, r, w, h, 14)
    m.step(sd, "yawed", **kw)
    sd = dataclasses.replace(sd, verts=moved_verts(sd))
    r.UpdateGeometry(verts=sd.verts)
    frame(P, r, w, h, 15)
    st, want = m.step(sd, "moved", **kw)
    return m, sd, st, want


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("name", ["cornell", "soup"])
def test_five_calls(P, pto, renderer, name, w, h):
    if name == "cornell":
        _, _, st, want = five_calls(P, pto, renderer, P.make_scene(P.native.PT_SCENE_CORNELL, 0, 3, w, h), w, h, 0, iterations=2)
    else:
        _, _, st, want = five_calls(P, pto, renderer, soup(P, w, h), w, h, 0, filter=False)
    if w * h > 1000:
        ids = want.history.g8[..., 7].view(np.uint32)
        assert (ids == tr.MISS).any() and (ids != tr.MISS).any() and st.paths <= (ids != tr.MISS).sum()
        assert st.gpu_ms > 0 and st.extend_ms > 0 and st.shade_ms > 0
        assert abs(st.gpu_ms - (st.extend_ms + st.shade_ms + st.other_ms)) < 1e-6


def test_lbvh_commit(P, pto, renderer):
    N = P.native
    w, h = 64, 48
    five_calls(P, pto, renderer, P.make_scene(N.PT_SCENE_CORNELL_GLASS, 0, 3, w, h), w, h, N.PT_BVH_WIDTH_4Q | N.PT_BVH_BUILD_LBVH)


@pytest.mark.parametrize("kw", [dict(match_ids=True), dict(max_history=1), dict(max_history=4), dict(plane_tolerance=0.001, normal_min=0.99),
                                dict(filter=True, guides_only=True), dict(edge_stops=False, iterations=3)],
                         ids=["match_ids", "max1", "max4", "tolerances", "guides_only", "no_edge_stops"])
def test_variants(P, pto, renderer, kw):
    w, h = 64, 48
    m, sd, _, want = five_calls(P, pto, renderer, P.make_scene(P.native.PT_SCENE_CORNELL, 0, 3, w, h), w, h, 0, **kw)
    for seed in (16, 17, 18):  # a still camera from here on: the lengths run into the cap
        frame(P, renderer, w, h, seed)
        _, want = m.step(sd, seed, **kw)
    cap = kw.get("max_history", 0) or 32
    if cap == 1:
        assert (want.length == 1).all() and same_bits(want.image, renderer.ReadFramebuffer())
    else:  # the move of call 5 restarted some pixels, the others have all 8 calls behind them
        assert want.length.max() == min(cap, 8) and want.length.min() == 1


def test_about_turn_has_no_history(P, pto, renderer):
    w, h = 64, 48
    sd = P.make_scene(P.native.PT_SCENE_CORNELL, 0, 3, w, h)
    renderer.SetScene(sd, 0)
    m = Mirror(P, pto, renderer)
    frame(P, renderer, w, h, 21)
    m.step(sd, "first", reset=True, filter=False)
    cam = tc.move_camera(sd.cam, yaw_deg=180.0)
    renderer.SetCamera(cam)
    frame(P, renderer, w, h, 22)
    st, want = m.step(tc.with_camera(sd, cam), "turned", filter=False)
    assert st.paths == 0 and (want.length == 1).all() and same_bits(want.image, renderer.ReadFramebuffer())


def test_still_camera_equals_accumulate(P, renderer):
    """8 frames of 1 spp with sample_offset = k and one seed under a still camera, max_history = 64: the accumulated image is the mean of
    the 8 samples, i.e. the framebuffer of one 8-spp frame, within 1e-5 max|c| (8 fused blends against one sum and division)."""
    w, h = 64, 48
    sd = P.make_scene(P.native.PT_SCENE_CORNELL, 0, 3, w, h)
    renderer.SetScene(sd, 0)
    for k in range(8):
        renderer.Params = P.make_params(w, h, spp=1, max_depth=6, seed=31, sample_offset=k)
        renderer.Render(0.0)
        renderer.DenoiseTemporal(max_history=64, reset=k == 0, filter=False)
    acc = renderer.ReadTemporal()
    hits = renderer.ReadGuides()[..., 7].view(np.uint32) != tr.MISS
    assert (renderer.ReadHistoryLength()[hits] == 8).all() and hits.mean() > 0.5
    renderer.Params = P.make_params(w, h, spp=8, max_depth=6, seed=31)
    renderer.Render(0.0)
    fb = renderer.ReadFramebuffer()
    assert np.abs(acc[..., :3] - fb[..., :3])[hits].max() <= 1e-5 * np.abs(fb[..., :3]).max()


def test_history_survives_other_calls(P, pto, renderer):
    """pt_render, pt_denoise and pt_trace_rays between two temporal calls change nothing; a size change restarts the history; the next
    pt_render expires the reads but not the history; a pt_denoise after a temporal call is what it is without one."""
    N = P.native
    w, h = 64, 48
    sd = P.make_scene(N.PT_SCENE_CORNELL_GLASS, 0, 3, w, h)
    renderer.SetScene(sd, 0)
    m = Mirror(P, pto, renderer)
    frame(P, renderer, w, h, 41)
    m.step(sd, "first", reset=True)
    frame(P, renderer, w, h, 77, streams=1)  # a frame nobody accumulates
    renderer.Denoise(iterations=3)
    renderer.TraceRays((np.zeros((5, 3), np.float32), np.tile(np.array([0.0, 0.0, -1.0], np.float32), (5, 1))))
    for read in (renderer.ReadTemporal, renderer.ReadHistoryLength):
        with pytest.raises(P.PtException) as e:
            read()
        assert e.value.status == N.PT_ERR_NOT_COMMITTED
    ptr, n = C.c_void_p(), C.c_uint64()
    assert N.lib.pt_temporal_device_ptr(renderer._ctx, C.byref(ptr), C.byref(n)) == N.PT_ERR_NOT_COMMITTED
    frame(P, renderer, w, h, 42)
    st, want = m.step(sd, "after render, denoise and trace")
    assert st.paths == (want.history.g8[..., 7].view(np.uint32) != tr.MISS).sum() > 0.5 * w * h
    assert N.lib.pt_temporal_device_ptr(renderer._ctx, C.byref(ptr), C.byref(n)) == N.PT_OK and n.value == w * h * 4 and ptr.value
    # pt_denoise after a temporal call: the same frame denoised with and without one in between
    frame(P, renderer, w, h, 43)
    renderer.Denoise()
    plain, plain_g = renderer.ReadDenoised(), renderer.ReadGuides()
    m.step(sd, "third")
    renderer.Denoise()
    assert same_bits(renderer.ReadDenoised(), plain) and same_bits(renderer.ReadGuides(), plain_g)
    renderer.ReadTemporal()  # (pt_denoise does not expire the accumulated image)
    # a size change restarts the history, on both sides
    sd2 = P.make_scene(N.PT_SCENE_CORNELL_GLASS, 0, 3, 32, 24)
    renderer.SetCamera(sd2.cam)
    frame(P, renderer, 32, 24, 44)
    st, want = m.step(sd2, "smaller")
    assert st.paths == 0 and (want.length == 1).all()
    frame(P, renderer, 32, 24, 45)
    st, _ = m.step(sd2, "smaller, second")
    assert st.paths > 0.5 * 32 * 24


def test_refusals_change_nothing(P, pto, renderer):
    """Every refusal returns its status and changes nothing: the previous results compare equal, and the next call's output is the
    checker's with the untouched history."""
    N, lib = P.native, P.native.lib
    w, h = 32, 24
    sd = P.make_scene(N.PT_SCENE_CORNELL, 0, 3, w, h)
    renderer.SetScene(sd, 0)
    m = Mirror(P, pto, renderer)
    frame(P, renderer, w, h, 51)
    m.step(sd, "first", reset=True)
    frame(P, renderer, w, h, 52)
    m.step(sd, "second")
    kept = [renderer.ReadTemporal(), renderer.ReadHistoryLength(), renderer.ReadDenoised(), renderer.ReadGuides()]

    def unchanged():
        now = [renderer.ReadTemporal(), renderer.ReadHistoryLength(), renderer.ReadDenoised(), renderer.ReadGuides()]
        return all(same_bits(a, b) for a, b in zip(now, kept))

    def status(**kw):
        with pytest.raises(P.PtException) as e:
            renderer.DenoiseTemporal(**kw)
        return e.value.status

    for kw in (dict(max_history=1048577), dict(plane_tolerance=-1.0), dict(plane_tolerance=float("nan")), dict(plane_tolerance=float("inf")),
               dict(normal_min=1.5), dict(normal_min=-0.25), dict(normal_min=float("nan")), dict(iterations=9), dict(sigma_color=-1.0),
               dict(sigma_depth=float("nan"))):
        assert status(**kw) == N.PT_ERR_INVALID_ARGUMENT, kw
    tp, dp = N.pt_temporal_params(), N.pt_denoise_params()
    ctx, scene = renderer._ctx, renderer._scene
    assert lib.pt_denoise_temporal(ctx, scene, None, C.byref(dp), None) == N.PT_ERR_INVALID_ARGUMENT
    assert lib.pt_denoise_temporal(ctx, scene, C.byref(N.pt_temporal_params(0, 0, 0, 4)), C.byref(dp), None) == N.PT_ERR_INVALID_ARGUMENT
    assert lib.pt_denoise_temporal(ctx, scene, C.byref(tp), C.byref(N.pt_denoise_params(0, 0, 0, 0, 0, 8)), None) == N.PT_ERR_INVALID_ARGUMENT
    assert lib.pt_denoise_temporal(ctx, None, C.byref(tp), C.byref(dp), None) == N.PT_ERR_INVALID_ARGUMENT
    assert unchanged()
    det, unc = C.c_void_p(), C.c_void_p()
    assert lib.pt_scene_create(None, C.byref(det)) == 0 and lib.pt_scene_create(ctx, C.byref(unc)) == 0
    other = P.Renderer(P.Window(w, h))
    other.Init()
    try:
        assert lib.pt_denoise_temporal(ctx, det, C.byref(tp), C.byref(dp), None) == N.PT_ERR_UNSUPPORTED
        other.SetScene(sd, 0)
        assert lib.pt_denoise_temporal(ctx, other._scene, C.byref(tp), C.byref(dp), None) == N.PT_ERR_UNSUPPORTED
        assert lib.pt_denoise_temporal(ctx, unc, C.byref(tp), C.byref(dp), None) == N.PT_ERR_NOT_COMMITTED
        assert lib.pt_denoise_temporal(other._ctx, other._scene, C.byref(tp), None, None) == N.PT_ERR_NOT_COMMITTED  # no frame there yet
    finally:
        lib.pt_scene_destroy(det)
        lib.pt_scene_destroy(unc)
        other.Dispose()
    assert unchanged()
    # frames a temporal call refuses: the reference sphere, and several ranks without assembly; the history outlives both
    renderer.Params = P.make_params(w, h, mode=N.PT_REFERENCE_SPHERE)
    renderer.Render(0.0)
    assert status() == N.PT_ERR_UNSUPPORTED
    renderer.Params = P.make_params(w, h, spp=1, max_depth=4, rank=0, nranks=2)
    renderer.Render(0.0)
    assert status() == N.PT_ERR_NOT_COMMITTED
    frame(P, renderer, w, h, 53)
    st, want = m.step(sd, "after the refusals")
    assert st.paths == (want.history.g8[..., 7].view(np.uint32) != tr.MISS).sum() and want.length.max() == 3


# displayed RMSE of temporal + filter over that of pt_denoise alone on the last frame, as measured on the device; the
# bound of the test is the midpoint between this ratio and 1
MEASURED_RATIO = {"C1": 0.375, "C4": 0.456}


@pytest.mark.parametrize("name", ["C1", "C4"])
def test_quality(P, renderer, name):
    """The experiment of tests/test_temporal.py on the device at 320 x 240 against a 4096-spp device frame of the last camera."""
    kind = {"C1": P.native.PT_SCENE_CORNELL, "C4": P.native.PT_SCENE_CORNELL_GLASS}[name]
    q = tc.device_quality(P, renderer, kind, 320, 240)
    alone, both = q["display"]
    print(name, q)
    assert both < alone
    assert both / alone <= (MEASURED_RATIO[name] + 1.0) / 2.0, (both, alone)
