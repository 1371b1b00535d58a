"""-m gpu: the camera's consumers on the device across the camera space (tests/camera_space.py has the cases and the scenes;
tests/test_camera_space.py shows without a device that the restated rule is sound and the cases sharp).

* The frame under every case and scene is the oracle's bit for bit on the device's own blob, rays and paths too, with the
  one-ray-per-lane kernel and with the lane-packing kernel; Cornell also with PT_FLAG_NEXT_EVENT. The §8.1 guides equal the checker's.
* The rectangle a frame reports (pt_stats.reserved[3], camera_space.reported_rect) equals camera_space.scene_rect64 of the same root
  bytes and spheres exactly, wherever no real-valued side of the reference lies within 1e-6 of an integer.
* Frames of one camera ray per sample (max_depth = 1, 64 spp) beside the rectangle; a camera change alone and a refit from device
  memory move the rectangle; §9's reprojection through general old cameras equals the temporal checker's."""
import dataclasses

import numpy as np
import pytest

import camera_space as cs
import denoise_checker as dc
import temporal_checker as tr
from frame_checks import check_denoise, check_nee
from pipelines import flags_of

pytestmark = pytest.mark.gpu

W, H = cs.W, cs.H
_cases = {}


def cases_of(P, name):
    """({case: scene data}, layout) of scene `name`, made once."""
    if name not in _cases:
        sd, layout = cs.scene(P, name)
        _cases[name] = (cs.cases(P, sd), layout)
    return _cases[name]


def reference(P, pto, r, sd, params):
    """The oracle's frame of `sd` on the renderer's current blob, and scene_rect64 of that blob's root and sd's spheres."""
    info = r.BvhInfo()
    nodes, tris = r.BvhRead()
    osc = pto.Scene(sd, (info.width, nodes, tris))
    assert osc.validate_bvh()[0] == 0
    ref, ost = pto.render(osc, params)
    return ref, ost, cs.scene_rect64(cs.root_slots(info.width, nodes), sd.spheres, sd.cam, params.width, params.height)


def same_frame(r, st, ref, ost, ctx):
    img = r.ReadFramebuffer()
    bad = np.argwhere((img != ref).any(axis=2))
    assert len(bad) == 0, (ctx, len(bad), bad[:4].tolist(), img[tuple(bad[0])].tolist(), ref[tuple(bad[0])].tolist())
    assert (st.rays, st.paths) == (ost.rays, ost.paths), (ctx, st.rays, ost.rays, st.paths, ost.paths)


def same_rectangle(st, want, ctx):
    """The reported rectangle is scene_rect64's, unless a side of the reference is tied; returns whether it was compared."""
    result, sides = want
    if cs.tied(sides, W, H):
        return False
    assert cs.reported_rect(st) == result, (ctx, cs.reported_rect(st), result, sides)
    return True


@pytest.mark.parametrize("case", cs.CASE_NAMES)
def test_frames_guides_and_rectangles(P, pto, renderer, case):
    """64 x 48, 4 spp, depth 4, 2 streams, every scene: both kernels' frames and rectangles, the guides, and Cornell's NEE frame."""
    N = P.native
    for name in cs.SCENES:
        table, layout = cases_of(P, name)
        sd = table[case]
        renderer.SetScene(sd, layout)
        p = P.make_params(W, H, spp=4, max_depth=4, streams=2)
        ref, ost, want = reference(P, pto, renderer, sd, p)
        for flag in flags_of("simple", "packed"):
            renderer.Params = P.make_params(W, H, spp=4, max_depth=4, streams=2, flags=flag)
            st = renderer.Render(0.0)
            same_frame(renderer, st, ref, ost, (case, name, flag))
            same_rectangle(st, want, (case, name, flag))
        check_denoise(P, pto, renderer, sd, (case, name), guides_only=True)
        if name == "cornell":
            renderer.Params = P.make_params(W, H, spp=4, max_depth=4, streams=2, flags=N.PT_FLAG_NEXT_EVENT)
            st, _ = check_nee(P, pto, renderer, sd, renderer.Params, (case, name, "nee"))
            same_rectangle(st, want, (case, name, "nee"))


def test_share_of_rectangles_compared(P, pto, renderer):
    """Every (case, scene) once more at 1 spp, on the device's blob: the rectangle where no side is tied, and the share left out for a
    tie, which may be one in ten at most. Measured: 0 of 138. Every resolving case reports a rectangle on some scene and every give-up
    case reports 0: the device agrees because it evaluates the rule, not because it gives up."""
    compared, resolved = 0, set()
    pairs = [(case, name) for name in cs.SCENES for case in cs.CASE_NAMES]
    for case, name in pairs:
        table, layout = cases_of(P, name)
        sd = table[case]
        renderer.SetScene(sd, layout)
        renderer.Params = p = P.make_params(W, H, spp=1, max_depth=2)
        st = renderer.Render(0.0)
        info = renderer.BvhInfo()
        want = cs.scene_rect64(cs.root_slots(info.width, renderer.BvhRead()[0]), sd.spheres, sd.cam, W, H)
        compared += same_rectangle(st, want, (case, name))
        got = cs.reported_rect(st)
        if got is not None:
            resolved.add(case)
        assert case not in cs.GIVE_UP or got is None, (case, name, got)
    left_out = len(pairs) - compared
    print(f"rectangles compared exactly: {compared} of {len(pairs)}, left out for a tie: {left_out}")
    assert left_out <= 0.1 * len(pairs), (left_out, len(pairs))
    assert resolved == set(cs.RESOLVING), sorted(set(cs.RESOLVING) - resolved)


@pytest.mark.parametrize("case", ["rolled", "off_centre", "skewed", "zoom_edge"])
def test_one_camera_ray_per_sample(P, pto, renderer, case):
    """max_depth = 1, 64 spp: every sample of every pixel beside the rectangle is a camera ray at a new jitter."""
    N = P.native
    for name in cs.SCENES:
        table, layout = cases_of(P, name)
        sd = table[case]
        renderer.SetScene(sd, layout)
        for flag, streams in zip(flags_of("simple", "packed"), (2, 4)):
            renderer.Params = p = P.make_params(W, H, spp=64, max_depth=1, streams=streams, flags=flag)
            ref, ost, want = reference(P, pto, renderer, sd, p)
            st = renderer.Render(0.0)
            same_frame(renderer, st, ref, ost, (case, name, flag))
            same_rectangle(st, want, (case, name, flag))


def test_camera_change_alone_and_refit(P, pto, renderer):
    """One commit of the tessellated Cornell box in layout 68; pt_scene_set_camera through five cases, then a refit from device memory
    under the last of them, then two more cameras: the rectangle follows each, and so does the frame (the frame-start template is
    keyed on geometry and remembers no rectangle)."""
    import torch
    table, layout = cases_of(P, "tess68")
    renderer.SetScene(table["default"], layout)
    p = P.make_params(W, H, spp=4, max_depth=4, streams=2)
    seen = []

    def frame(sd, ctx):
        renderer.Params = p
        ref, ost, want = reference(P, pto, renderer, sd, p)
        st = renderer.Render(0.0)
        same_frame(renderer, st, ref, ost, ctx)
        assert same_rectangle(st, want, ctx), ("tied", ctx)
        seen.append(cs.reported_rect(st))

    for case in ("default", "rolled", "anisotropic", "inside", "mirrored", "wide"):
        renderer.SetCamera(table[case].cam)
        frame(table[case], case)
    assert len(set(seen)) == len(seen) and None in seen, seen  # six different answers, one of them "nothing resolved"
    sd = table["wide"]
    moved = dataclasses.replace(sd, verts=(np.array(sd.verts).reshape(-1, 3, 3) + np.float32([0.9, -0.4, 0.0])).reshape(-1, 9))
    renderer.UpdateGeometry(verts=torch.as_tensor(moved.verts, device="cuda"))
    frame(moved, "wide, moved")
    assert seen[-1] != seen[-2], seen[-2:]
    for case in ("skewed", "default"):
        renderer.SetCamera(table[case].cam)
        frame(dataclasses.replace(moved, cam=table[case].cam), (case, "moved"))


@pytest.mark.parametrize("motion", [False, True])
@pytest.mark.parametrize("case", cs.TEMPORAL_CASES)
def test_temporal_through_general_cameras(P, pto, renderer, case, motion):
    """Two frames of Cornell, the second through the case's camera moved by move_camera, each followed by pt_denoise_temporal without
    the filter: the accumulated image, the lengths and stats.paths equal the temporal checker's bit for bit, with and without
    PT_TEMPORAL_MOTION (the geometry is unchanged, so §9.1 reduces to §9). Most hit pixels take history through the old camera."""
    sd = P.make_scene(P.native.PT_SCENE_CORNELL, 0, 3, W, H)
    old, new = cs.camera_pair(P, sd, case)
    renderer.SetScene(old, 0)
    hist = None
    for k, s in enumerate((old, new)):
        renderer.SetCamera(s.cam)
        renderer.Params = P.make_params(W, H, spp=4, max_depth=4, streams=2, seed=11 + k)
        renderer.Render(0.0)
        g = dc.guides(pto, pto.Scene(s), W, H)
        want = tr.accumulate(renderer.ReadFramebuffer(), g, s.cam, hist, tr.params(flags=0 if k else tr.RESET))
        st = renderer.DenoiseTemporal(reset=k == 0, filter=False, motion=motion)
        img, length = renderer.ReadTemporal(), renderer.ReadHistoryLength()
        bad = np.argwhere((img.view(np.uint32) != want.image.view(np.uint32)).any(axis=2))
        assert len(bad) == 0, (case, k, len(bad), bad[:3].tolist(), img[tuple(bad[0])].tolist(), want.image[tuple(bad[0])].tolist())
        bad = np.argwhere(length.view(np.uint32) != want.length.view(np.uint32))
        assert len(bad) == 0, (case, k, len(bad), bad[:3].tolist())
        assert st.paths == want.taken == int((length > 1).sum()) and st.rays == W * H, (case, k, st.paths, want.taken)
        assert np.array_equal(renderer.ReadGuides().view(np.uint32), g.view(np.uint32)), (case, k)
        hist = want.history
    hits = g[..., 7].view(np.uint32) != tr.MISS
    assert want.taken > 0.5 * hits.sum(), (case, want.taken, hits.sum())
