"""-m gpu: the thin-lens camera (pt_scene_set_lens, docs/SPEC.md §3.1) on the device against the scalar checker of tests/lens_ref/.

Frames are compared bit for bit, rays and paths included, along the axes a lens can break: the scenes (all material kinds with spheres;
a Lambert-only soup, which the lens instantiation still shades with all-kinds code; a tessellated box with next-event estimation), the
node layouts and builders, the ways samples are dealt to streams (regeneration in place, empty streams, a sample offset), jitter, three
lenses from almost a pinhole to an aperture wider than the focus distance, and schedules under which a path and its origin cross
launches. Then the environment seen through a lens, what must not have moved, and the call rules."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import camera_space as cs
import env_checker as ec
import lens_checker as lc
import schedules as sch
from lens_device import check
from pipelines import RUNNABLE, refused
from trace_support import H, LAYOUTS, W

pytestmark = pytest.mark.gpu

LENSES = [(0.05, 2.5), (1e-3, 1e3), (0.5, 0.25)]
SPLITS = [(5, 1, 0), (7, 3, 0), (2, 4, 0), (4, 2, 3)]  # (spp, streams, sample_offset)


def cam_copy(cam):
    c = type(cam)()
    C.memmove(C.byref(c), C.byref(cam), C.sizeof(c))
    return c


def with_jitter(sd, jitter):
    cam = cam_copy(sd.cam)
    cam.jitter = jitter
    return dataclasses.replace(sd, cam=cam)


@pytest.fixture(scope="module")
def scenes(P):
    N = P.native
    return {"glass": (P.make_scene(N.PT_SCENE_CORNELL_GLASS, 0, 3, W, H), False),
            "soup": (dataclasses.replace(P.make_scene(N.PT_SCENE_TRIANGLE_SOUP, 300, 3, W, H), sky=np.float32([0.4, 0.6, 0.9])), False),
            "tess": (P.make_scene(N.PT_SCENE_CORNELL_TESS, 2000, 3, W, H), True)}


def params_of(P, nee, split=(5, 1, 0), **kw):
    spp, streams, offset = split
    p = P.make_params(W, H, spp=spp, streams=streams, sample_offset=offset, max_depth=6, rr_start=2, **kw)
    if nee:
        p.flags |= P.native.PT_FLAG_NEXT_EVENT
    return p


def frame(P, pto, r, scenes, name, lens, split, jitter, ctx, width=None):
    """Commit (width given) or keep the scene, set the lens, render and check one frame."""
    sd, nee = scenes[name]
    sd = with_jitter(sd, jitter)
    if width is not None:
        r.SetScene(sd, width)
    else:
        r.SetCamera(sd.cam)
    r.SetLens(*lens)
    r.Params = params_of(P, nee, split)
    return check(P, pto, r, name, sd, lens, r.Params, ctx)


# ------------------------------------------------------------------------------------------------------------- 1. parity with lr_render
def test_layouts_and_builders(P, pto, renderer, scenes):
    """The five layouts on the glass box with in-place regeneration; both builders on the NEE box."""
    for width in LAYOUTS:
        frame(P, pto, renderer, scenes, "glass", LENSES[0], SPLITS[1], 1, ("layout", width), width=width)
    for build in (0, P.native.PT_BVH_BUILD_LBVH):
        frame(P, pto, renderer, scenes, "tess", LENSES[0], SPLITS[1], 1, ("builder", build), width=68 | build)


@pytest.mark.parametrize("name", ["glass", "soup", "tess"])
def test_sample_splits_and_jitter(P, pto, renderer, scenes, name):
    """(spp, streams, sample_offset): one stream; regeneration in place; empty streams (dense generate mode); an offset. Each with and
    without jitter — the lens point is drawn either way."""
    first = True
    for k, split in enumerate(SPLITS):
        for jitter in (0, 1):
            frame(P, pto, renderer, scenes, name, LENSES[k % 3], split, jitter, (name, split, jitter), width=0 if first else None)
            first = False


@pytest.mark.parametrize("name", ["glass", "tess"])
def test_lenses(P, pto, renderer, scenes, name):
    """Almost a pinhole focused far away, a moderate lens, an aperture twice the focus distance."""
    first = True
    for lens in LENSES:
        for jitter in (0, 1):
            frame(P, pto, renderer, scenes, name, lens, SPLITS[3], jitter, (name, lens, jitter), width=0 if first else None)
            first = False


@pytest.mark.parametrize("schedule", ["default", "pass", "loops1", "loops2", "loops4"])
def test_schedules(P, pto, scenes, schedule):
    """One ray per launch and no finish mode: a path is stored by one launch and loaded by the next, its origin with it, and a
    regenerated sample gets its own. The default schedule is the control that says the others added launches."""
    r = sch.tuned(P, schedule, W, H)
    d = sch.tuned(P, "default", W, H) if schedule != "default" else None
    try:
        for name in ("glass", "tess"):
            st = frame(P, pto, r, scenes, name, LENSES[0], SPLITS[1], 1, (schedule, name), width=0)
            if d is not None:
                dst = frame(P, pto, d, scenes, name, LENSES[0], SPLITS[1], 1, ("default", name), width=0)
                slots = W * H * min(SPLITS[1][1], SPLITS[1][0])
                sch.check_stats(schedule, st, dst, slots, (schedule, name))
    finally:
        r.Dispose()
        if d is not None:
            d.Dispose()


# ------------------------------------------------------------------------------------------------------------------ 2. environment x lens
def test_environment_through_the_lens(P, pto, renderer):
    """Every camera ray misses: a pixel is the f32 sum, in sample order, of the map's texels at encode(d) of the checker's lens rays,
    times 1 / spp, exactly — with and without NEE (no vertex, no light sample)."""
    n, spp, lens = 8, 3, LENSES[2]
    env = ec.distinct(n)
    for jitter in (0, 1):
        sd = lc.all_miss_scene(P, W, H, jitter)
        renderer.SetScene(dataclasses.replace(sd, environment=env), 0)
        renderer.SetLens(*lens)
        want = np.zeros((H, W, 3), np.float32)
        seed = params_of(P, False).seed
        for y in range(H):
            for x in range(W):
                acc = np.zeros(3, np.float32)
                for s in range(spp):
                    _, d = lc.camera_ray(pto, sd.cam, lens, x, y, pto.lib.pto_path_key(seed, y * W + x, s))
                    i, j, _ = ec.encode(d, n)
                    acc = acc + env[j, i]
                want[y, x] = acc * (np.float32(1.0) / np.float32(spp))
        for nee in (False, True):
            renderer.Params = params_of(P, nee, (spp, 1, 0))
            st = renderer.Render(0.0)
            img = renderer.ReadFramebuffer()
            assert np.array_equal(img[..., :3], want), (jitter, nee)
            assert st.rays == st.paths == W * H * spp and st.reserved[0] == 1
        assert len(np.unique(want.reshape(-1, 3), axis=0)) > 8  # the aperture spreads a pixel's rays over many texels


def test_environment_nee_lens_on_two_layouts(P, pto, renderer, scenes):
    sd = dataclasses.replace(ec.scene(P, "cornell", W, H), environment=ec.sun_sky(P))
    frames = []
    for width in (2, 68):
        renderer.SetScene(sd, width)
        renderer.SetLens(*LENSES[0])
        renderer.Params = params_of(P, True, SPLITS[1])
        st = renderer.Render(0.0)
        frames.append((renderer.ReadFramebuffer(), st.rays, st.paths))
        assert np.isfinite(frames[-1][0]).all() and st.reserved[0] == 1
    assert np.array_equal(frames[0][0], frames[1][0]) and frames[0][1:] == frames[1][1:]
    renderer.ClearLens()
    renderer.Render(0.0)
    assert not np.array_equal(renderer.ReadFramebuffer(), frames[1][0])  # the lens was there


# ----------------------------------------------------------------------------------------------------------------- 3. nothing else moved
def _stats_key(st, forced):
    return (st.rays, st.paths, st.node_visits, st.tri_tests, st.sphere_tests, st.reserved[3]) + ((st.reserved[0],) if forced else ())


@pytest.mark.parametrize("pipe", RUNNABLE, ids=[p.name for p in RUNNABLE])
def test_radius_zero_and_cleared_lens_are_no_lens(P, pto, renderer, scenes, pipe):
    """Every runnable pipeline: the frame and its pt_stats without the call, with radius 0, and after ClearLens(), each on a fresh
    commit (so that the scene's kernel probe starts alike). reserved[0] is compared where the pipeline forces a kernel: the probe's
    choice is a measurement."""
    sd = scenes["glass"][0]
    got = []
    for step in ("none", "zero", "cleared"):
        renderer.SetScene(sd, 0)
        if step == "zero":
            renderer.SetLens(0.0, 3.0)
        elif step == "cleared":
            renderer.SetLens(0.2, 3.0)
            renderer.ClearLens()
        p = params_of(P, False, SPLITS[1])
        p.flags |= pipe.flags
        renderer.Params = p
        st = renderer.Render(0.0)
        got.append((renderer.ReadFramebuffer(), _stats_key(st, pipe.kernel is not None)))
    for img, key in got[1:]:
        assert np.array_equal(img, got[0][0]) and key == got[0][1], (pipe.name, key, got[0][1])


def test_queries_gathers_and_guides_do_not_see_the_lens(P, pto, renderer, scenes):
    sd = scenes["glass"][0]
    renderer.SetScene(sd, 0)
    rng = np.random.default_rng(3)
    o = rng.uniform(-0.5, 0.5, (256, 3)).astype(np.float32)
    d = rng.normal(size=(256, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)

    def everything():
        renderer.Params = params_of(P, False, SPLITS[0])
        renderer.Render(0.0)
        renderer.Denoise(iterations=1)
        hits = renderer.TraceRays((o, d))[0]
        E, vis, bent, _ = renderer.Gather(o, d, samples=16, seed=7)
        return [np.ascontiguousarray(a).view(np.uint32).copy() for a in (renderer.ReadGuides(), hits, E, vis, bent)]

    want = everything()
    renderer.SetLens(*LENSES[2])
    got = everything()
    for a, b in zip(want, got):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------------------------------- 4. call rules
def test_set_after_commit_survives_commit_and_update(P, pto, renderer, scenes):
    sd, nee = scenes["tess"]
    renderer.SetScene(sd, 0)
    renderer.Params = params_of(P, nee, SPLITS[1])
    renderer.SetLens(*LENSES[0])                       # after the commit: no new commit needed
    assert renderer.Lens() == tuple(np.float32(LENSES[0]).tolist())
    check(P, pto, renderer, "tess", sd, LENSES[0], renderer.Params, "after commit")
    with pytest.raises(P.PtException):
        renderer.SetLens(-1.0, 2.0)                    # refused: the lens stays
    assert P.native.lib.pt_scene_commit(renderer._scene, 68) == 0
    check(P, pto, renderer, "tess", sd, LENSES[0], renderer.Params, "after a second commit")
    v2 = sd.verts.copy()
    v2[:, 1::3] *= 0.9
    renderer.UpdateGeometry(verts=v2)
    moved = dataclasses.replace(sd, verts=v2)
    check(P, pto, renderer, "tess squashed", moved, LENSES[0], renderer.Params, "after update")
    renderer.SetCamera(with_jitter(moved, 0).cam)      # ... and pt_scene_set_camera
    check(P, pto, renderer, "tess squashed", with_jitter(moved, 0), LENSES[0], renderer.Params, "after set_camera")


def test_accumulate_and_virtual_ranks(P, pto, renderer, scenes):
    N = P.native
    sd, nee = scenes["glass"]
    renderer.SetScene(sd, 0)
    renderer.SetLens(*LENSES[0])
    renderer.Params = params_of(P, nee, (5, 2, 0))
    whole = check(P, pto, renderer, "glass", sd, LENSES[0], renderer.Params, "whole")
    want = renderer.ReadFramebuffer()
    rays = 0
    for spp, offset in ((3, 0), (2, 3)):
        p = params_of(P, nee, (spp, 2, offset))
        if offset:
            p.flags |= N.PT_FLAG_ACCUMULATE
        renderer.Params = p
        rays += renderer.Render(0.0).rays
    assert np.array_equal(renderer.ReadFramebuffer(), want) and rays == whole.rays
    for ranks in (2, 3):
        with P.Comm([renderer] * ranks, root=ranks - 1) as comm:
            stats = comm.Render(params_of(P, nee, (5, 2, 0)))
            assert sum(s.rays for s in stats) == whole.rays and sum(s.paths for s in stats) == whole.paths
            assert np.array_equal(renderer.ReadFramebuffer(), want), ranks


def test_a_lens_frame_resolves_no_sky_pixels(P, pto, renderer):
    sd = cs.cases(P, cs.scene(P, "triangle")[0])["default"]
    renderer.SetScene(sd, 0)
    renderer.Params = P.make_params(cs.W, cs.H, spp=2, max_depth=4)
    assert renderer.Render(0.0).reserved[3] != 0       # the pinhole frame resolves pixels
    renderer.SetLens(*LENSES[0])
    st = renderer.Render(0.0)
    assert st.reserved[3] == 0 and st.reserved[0] == 1
    ref, cst, _ = lc.render(pto, pto.Scene(sd), renderer.Params, lens=LENSES[0])
    assert np.array_equal(renderer.ReadFramebuffer(), ref) and st.rays == cst.ext_rays


def test_refused_pipelines_and_degenerate_basis(P, pto, renderer, scenes):
    """What an environment frame is refused with, a lens frame is refused with, and the message names the lens."""
    N = P.native
    sd, _ = scenes["glass"]
    renderer.SetScene(sd, 0)
    renderer.SetLens(*LENSES[0])
    for nee in (False, True):
        for flags in [r.flags for r in refused("env")]:
            p = params_of(P, nee, SPLITS[0])
            p.flags |= flags
            renderer.Params = p
            with pytest.raises(P.PtException, match="lens") as e:
                renderer.Render(0.0)
            assert e.value.status == N.PT_ERR_UNSUPPORTED, flags
    tuning = renderer.GetTuning().extend_kernel
    try:
        for k in [r.tuned_kernel for r in refused("env", tuned=True)]:
            renderer.SetTuning(extend_kernel=k)
            renderer.Params = params_of(P, False, SPLITS[0])
            with pytest.raises(P.PtException, match="lens") as e:
                renderer.Render(0.0)
            assert e.value.status == N.PT_ERR_UNSUPPORTED, k
    finally:
        renderer.SetTuning(extend_kernel=tuning)
    flat = cam_copy(sd.cam)
    flat.right[:] = (0.0, 0.0, 0.0)
    renderer.SetCamera(flat)
    renderer.Params = params_of(P, False, SPLITS[0])
    with pytest.raises(P.PtException) as e:
        renderer.Render(0.0)
    assert e.value.status == N.PT_ERR_INVALID_ARGUMENT
    renderer.SetCamera(sd.cam)
    p = params_of(P, False, SPLITS[0])
    p.flags |= N.PT_FLAG_EXTEND_SIMPLE | N.PT_FLAG_PROFILE_KERNELS  # the kernel these frames run on, forced, and timed: accepted
    renderer.Params = p
    check(P, pto, renderer, "glass", sd, LENSES[0], p, "after refusals")
