"""-m gpu: next-event estimation (docs/SPEC.md §7) and environment-map frames (§11) against their scalar checkers (tests/nee_ref/,
tests/env_ref/) under every launch schedule of tests/schedules.py.

These frames run on k_extend instantiations of their own and carry more from one launch to the next than a plain frame: the NEE flags
and the shadow ray's tmax in the .w words of the stored ray, the waiting extension ray and the pending radiance per slot, a `bounces`
that counts rays, a doubled drain bound. A launch boundary can fall between a vertex's shadow ray and its extension ray, and a re-pack
can move a queue entry whose slot has a shadow ray pending. No scheduling knob may change a pixel (include/ptrt.h pt_tuning).

The measurement that motivates the module, on one MI355X: the `lights` scene at 48 x 36 with nee_params(spp=4, max_depth=8, streams=2),
a frame of test_gpu_nee.py, under the default tuning gives iterations = 3 (one launch and the host's lag) and reserved[2] = 3456, which is
the 1728 pixels x 2 streams that the first launch starts: finish_below = 4096 per shard runs every path to its end inside that launch
and no path state is ever loaded. The same frame under `pass` (bounces = 1, finish_below = 0) takes 30 iterations and loads or starts
26890 states for the same 27610 rays. Every NEE and ENV frame of the suite before this module was of the first kind.

Every frame is compared bit for bit with the checker's, which does not depend on the schedule (one reference per scene, frame and
estimator, computed once per module): pixels, rays = extension + shadow rays, paths, and the one-ray-per-lane kernel in pt_stats. Every
schedule with finish_below = 0 must also show that path states crossed launches (schedules.check_stats), against the same frame under
the default schedule on the session renderer, whose tuning is never touched; every schedule renders on a context of its own."""
import dataclasses

import numpy as np
import pytest

import adversarial_scenes as adv
import camera_space as cs
import env_checker as ec
import nee_checker as nc
import schedules as sc
from frame_checks import check_against_oracle, check_nee
from pipelines import named_flags
from trace_support import H, LAYOUTS, W

pytestmark = pytest.mark.gpu

# k4: the streams end at different iterations (7 samples over 4 streams, Russian roulette), so carried queues have holes; k1: one stream
# alone; drain: sweep 3's frame without roulette; whole: the 16 samples that sweep 4 also renders as four accumulating calls
FRAMES = {"k4": dict(spp=7, max_depth=8, streams=4), "k1": dict(spp=8, max_depth=8, streams=1),
          "drain": dict(spp=2, streams=1, max_depth=6, rr_start=6), "whole": dict(spp=16, max_depth=8, streams=4)}
NEE_SCENES = ("lights", "grazing", "glass")
ENV_SCENES = ("soup", "cornell", "glass")

_scenes, _refs, _defaults = {}, {}, {}


def scene(P, kind, name):
    """The scenes of the sweeps, made once: ("nee", ..) of test_gpu_nee.py, ("env", ..) of test_gpu_env.py under ec.sun_sky."""
    if (kind, name) not in _scenes:
        if kind == "nee":
            sd = {"lights": lambda: nc.many_lights_scene(P, W, H), "grazing": lambda: nc.grazing_scene(P, W, H),
                  "glass": lambda: P.make_scene(P.native.PT_SCENE_CORNELL_GLASS, 0, 3, W, H),
                  "cornell": lambda: P.make_scene(P.native.PT_SCENE_CORNELL, 0, 3, W, H)}[name]()
        else:
            if "sun" not in _scenes:
                _scenes["sun"] = ec.sun_sky(P)
            sd = dataclasses.replace(ec.scene(P, name, W, H), environment=_scenes["sun"])
        _scenes[(kind, name)] = sd
    return _scenes[(kind, name)]


def params_of(P, nee, **kw):
    p = P.make_params(W, H, **kw)
    if nee:
        p.flags |= P.native.PT_FLAG_NEXT_EVENT
    return p


def reference(pto, kind, name, sd, params, frame, nee):
    """(frame, stats) of the checker for scene (kind, name) under `params` = FRAMES[frame] with or without NEE. Once per module."""
    k = (kind, name, frame, nee)
    if k not in _refs:
        if kind == "nee":
            ref, cst, _ = nc.render(pto, pto.Scene(sd), params)
        else:
            ref, cst, _ = ec.render(pto, pto.Scene(sd), params, env=sd.environment, flags=ec.NEE if nee else 0)
        ref.setflags(write=False)
        _refs[k] = (ref, cst)
    return _refs[k]


def default_stats(renderer, sd, layout, params, key):
    """pt_stats of the same frame under the default schedule, on the session renderer; once per (frame, layout)."""
    if key not in _defaults:
        renderer.SetScene(sd, layout)
        renderer.Params = params
        _defaults[key] = renderer.Render(0.0)
    return _defaults[key]


def live_slots(params):
    """The path states a frame's first launch starts: one per pixel and sample stream that has a sample."""
    return params.width * params.height * min(max(params.streams, 1), params.spp)


def rays_per_sample(params, nee, cst):
    """The most rays that the samples of this frame are held to need, for schedules.can_cross: max_depth extension rays, and with NEE a
    shadow ray at every vertex below max_depth. Per the checker, the sun-lit soup at this size is sky but for a few dozen rays (its
    triangles are smaller than a pixel): there a sample is its camera ray, and only a schedule that cuts between a stream's samples
    carries a state over."""
    if cst.ext_rays + cst.shadow_rays <= 1.05 * cst.paths:
        return 1
    return 2 * params.max_depth - 1 if nee else params.max_depth


def same_frame(img, st, ref, cst, ctx):
    assert np.isfinite(img).all(), ctx
    bad = np.argwhere((img != ref).any(axis=2))
    assert len(bad) == 0, (ctx, len(bad), bad[:4].tolist(), img[tuple(bad[0])].tolist(), ref[tuple(bad[0])].tolist())
    assert st.rays == cst.ext_rays + cst.shadow_rays, (ctx, st.rays, cst.ext_rays, cst.shadow_rays)
    assert st.paths == cst.paths and st.reserved[0] == 1, (ctx, st.paths, cst.paths, st.reserved[0])


def hold(P, pto, renderer, r, name, kind, scene_name, layout, nee, frame="k4"):
    """Renderer `r` (schedule `name`) renders scene (kind, scene_name) in `layout`: the checker's frame, and the schedule's stats."""
    sd = scene(P, kind, scene_name)
    params = params_of(P, nee, **FRAMES[frame])
    ctx = (name, kind, scene_name, layout, nee, frame)
    r.SetScene(sd, layout)
    r.Params = params
    st = r.Render(0.0)
    ref, cst = reference(pto, kind, scene_name, sd, params, frame, nee)
    same_frame(r.ReadFramebuffer(), st, ref, cst, ctx)
    assert (cst.shadow_rays > 0) == nee, ctx
    dst = default_stats(renderer, sd, layout, params, ctx[1:])
    crossing = sc.can_cross(name, params.spp, params.streams, rays_per_sample(params, nee, cst))
    print(f"{ctx}: iterations {st.iterations} (default {dst.iterations}), states {st.reserved[2]} (default {dst.reserved[2]}), "
          f"re-packs {st.reserved[1]}, live slots {live_slots(params)}, must cross {crossing}")
    sc.check_stats(name, st, dst, live_slots(params), ctx, crossing)
    return st


# ------------------------------------------------------------------------------------------------------------------------ sweep 1: NEE
@pytest.mark.parametrize("name", sc.NAMES)
def test_nee_under_every_schedule(P, pto, renderer, name):
    """Many lights, grazing lights and the glass Cornell on BVH2 and BVH4Q; and one stream alone (8 samples one after the other)."""
    r = sc.tuned(P, name, W, H)
    try:
        for scene_name in NEE_SCENES:
            for layout in (2, 68):
                hold(P, pto, renderer, r, name, "nee", scene_name, layout, True)
        hold(P, pto, renderer, r, name, "nee", "lights", 68, True, "k1")
        hold(P, pto, renderer, r, name, "nee", "glass", 2, True, "k1")
    finally:
        r.Dispose()


@pytest.mark.parametrize("scene_name", NEE_SCENES)
def test_nee_one_ray_per_launch_on_every_layout(P, pto, renderer, scene_name):
    """`pass` on every layout with both builders: each k_extend<L, .., NEE> stores and reloads the NEE words."""
    r = sc.tuned(P, "pass", W, H)
    try:
        for layout in LAYOUTS:
            for build in (0, P.native.PT_BVH_BUILD_LBVH):
                hold(P, pto, renderer, r, "pass", "nee", scene_name, layout | build, True)
    finally:
        r.Dispose()


# ------------------------------------------------------------------------------------------------------------------------ sweep 2: ENV
@pytest.mark.parametrize("name", sc.NAMES)
def test_env_under_every_schedule(P, pto, renderer, name):
    """The sun-lit soup, Cornell and glass Cornell on BVH4Q, plain and with NEE (the map and the triangles both sampled); and one stream
    alone, whose 8 samples one after the other are more rays than any schedule's launch: a plain path is at most max_depth = 8 rays, so the
    two samples of a stream of the first frame fit the 16 rays of `long`, and the soup's (sky but for a few) fit every launch but `pass`'s."""
    r = sc.tuned(P, name, W, H)
    try:
        for scene_name in ENV_SCENES:
            for nee in (False, True):
                hold(P, pto, renderer, r, name, "env", scene_name, 68, nee)
        for scene_name, nee in (("soup", False), ("cornell", False), ("cornell", True)):
            hold(P, pto, renderer, r, name, "env", scene_name, 68, nee, "k1")
    finally:
        r.Dispose()


@pytest.mark.parametrize("scene_name", ENV_SCENES)
def test_env_one_ray_per_launch_on_every_layout(P, pto, renderer, scene_name):
    """`pass` on every layout, plain and with NEE: each k_extend<L, .., SHADE_INLINE, [NEE,] ENV> stores and reloads its state."""
    r = sc.tuned(P, "pass", W, H)
    try:
        for layout in LAYOUTS:
            for nee in (False, True):
                hold(P, pto, renderer, r, "pass", "env", scene_name, layout, nee)
    finally:
        r.Dispose()


# ------------------------------------------------------------------------------------------------------------ sweep 3: the drain bound
@pytest.mark.parametrize("kind", ["nee", "env"])
def test_drain_bound(P, pto, renderer, kind):
    """No roulette (rr_start = max_depth = 6), one stream of 2 samples, one ray per launch: a slot whose samples both reach the depth cut
    with a light sample at every vertex below it needs 2 x (6 + 5) = 22 launches, and the host gives up after spp x max_depth x 2 (+ its
    lag). The frame is the checker's and Render does not raise "wavefront loop did not drain"."""
    r = sc.tuned(P, "pass", W, H)
    try:
        st = hold(P, pto, renderer, r, "pass", kind, "cornell", 0, True, "drain")
        _, cst = _refs[(kind, "cornell", "drain", True)]
        print(f"drain {kind}: {(cst.ext_rays + cst.shadow_rays) / cst.paths:.2f} rays per path, {st.iterations} iterations")
        assert st.iterations >= 22, (kind, st.iterations)  # some slot does take the longest way
    finally:
        r.Dispose()


# ------------------------------------------------------------------------------------- sweep 4: progressive frames, ranks, sky pixels
CASES4 = [("nee", "lights"), ("env", "cornell")]


@pytest.mark.parametrize("kind,scene_name", CASES4, ids=["nee", "env+nee"])
def test_progressive_under_pass(P, pto, renderer, kind, scene_name):
    """Four accumulate calls of 4 spp = one call of 16 spp = the checker's frame, one ray per launch."""
    N = P.native
    r = sc.tuned(P, "pass", W, H)
    try:
        whole = hold(P, pto, renderer, r, "pass", kind, scene_name, 0, True, "whole")
        want = r.ReadFramebuffer()
        rays = 0
        for k in range(4):
            p = params_of(P, True, spp=4, max_depth=8, streams=4, sample_offset=4 * k)
            if k:
                p.flags |= N.PT_FLAG_ACCUMULATE
            r.Params = p
            st = r.Render(0.0)
            assert st.reserved[2] > live_slots(p), (k, st.reserved[2])
            rays += st.rays
        assert np.array_equal(r.ReadFramebuffer(), want) and rays == whole.rays, (rays, whole.rays)
    finally:
        r.Dispose()


@pytest.mark.parametrize("kind,scene_name", [("nee", "lights"), ("env", "glass")], ids=["nee", "env+nee"])
def test_ranks_under_pass(P, pto, renderer, kind, scene_name):
    """Three virtual ranks on one context, one ray per launch, assemble the single-rank frame, which is the checker's."""
    r = sc.tuned(P, "pass", W, H)
    try:
        one = hold(P, pto, renderer, r, "pass", kind, scene_name, 0, True)
        want = r.ReadFramebuffer()
        params = params_of(P, True, **FRAMES["k4"])
        with P.Comm([r] * 3, root=2) as comm:
            stats = comm.Render(params)
            assert sum(s.rays for s in stats) == one.rays and sum(s.paths for s in stats) == one.paths
            assert sum(s.reserved[2] for s in stats) > live_slots(params)
            assert np.array_equal(r.ReadFramebuffer(), want)
    finally:
        r.Dispose()


def test_ranks_with_tiles_of_their_own_under_pass(P, pto, renderer):
    """48 x 36 is one 64 x 64 tile, which rank 0 owns. At 100 x 130 (2 x 3 tiles, the right column and the bottom row partial; tile t is
    rank t % 3's) each of three ranks renders two tiles in which paths go on after the camera ray, one ray per launch: every rank carries
    states across launches, the rays and paths add up and the assembled frame is the checker's."""
    w, h = 100, 130
    sd = nc.many_lights_scene(P, w, h)
    params = P.make_params(w, h, flags=P.native.PT_FLAG_NEXT_EVENT, **FRAMES["k4"])
    ref, cst, _ = nc.render(pto, pto.Scene(sd), params)
    r = sc.tuned(P, "pass", w, h)
    try:
        r.SetScene(sd, 0)
        r.Params = params
        one = r.Render(0.0)
        same_frame(r.ReadFramebuffer(), one, ref, cst, "one rank")
        sc.check_stats("pass", one, default_stats(renderer, sd, 0, params, "100 x 130"), live_slots(params), "100 x 130")
        with P.Comm([r] * 3, root=2) as comm:
            stats = comm.Render(params)
            got = [(s.paths, s.rays, s.reserved[2], s.iterations) for s in stats]
            print("ranks (paths, rays, states, iterations):", got)
            for paths, rays, states, _ in got:
                assert rays > paths > 0, got  # the rank owns pixels that see the scene ...
                assert states > paths // params.spp * params.streams, got  # ... so the states of its slots outlive their first launch
            assert sum(s.rays for s in stats) == one.rays and sum(s.paths for s in stats) == one.paths
            assert np.array_equal(r.ReadFramebuffer(), ref)
    finally:
        r.Dispose()


def test_sky_pixels_under_pass(P, pto, renderer):
    """A camera-space case on Cornell that leaves sky pixels, with NEE, one ray per launch: sky-pixel slots are holes of the first launch
    only (kernels.hip queued_slot), every later launch takes the queue as it finds it. The checker's frame, and the rectangle that
    camera_space.scene_rect64 derives in float64 from the blob's root."""
    sd0, layout = cs.scene(P, "cornell")
    table = cs.cases(P, sd0)
    r = sc.tuned(P, "pass", cs.W, cs.H)
    try:
        for case in cs.RESOLVING:  # the first resolving case whose rectangle is a proper one with no side tied
            sd = table[case]
            r.SetScene(sd, layout)
            info = r.BvhInfo()
            result, sides = cs.scene_rect64(cs.root_slots(info.width, r.BvhRead()[0]), sd.spheres, sd.cam, cs.W, cs.H)
            if isinstance(result, tuple) and not cs.tied(sides, cs.W, cs.H):
                break
        else:
            pytest.fail("no resolving case leaves a rectangle on Cornell")
        params = P.make_params(cs.W, cs.H, spp=7, max_depth=8, streams=4, flags=P.native.PT_FLAG_NEXT_EVENT)
        r.Params = params
        st, cst = check_nee(P, pto, r, sd, params, (case, "pass"))
        assert st.reserved[0] == 1 and cs.reported_rect(st) == result, (case, cs.reported_rect(st), result)
        x0, x1, y0, y1 = result
        assert (x1 - x0) * (y1 - y0) < cs.W * cs.H  # there are sky pixels
        sc.check_stats("pass", st, default_stats(renderer, sd, layout, params, ("sky", case)), live_slots(params), case)
    finally:
        r.Dispose()


# --------------------------------------------------------------------------------------------- sweep 5: stack spill across launches
@pytest.mark.parametrize("pipeline,flags", named_flags("simple", "packed", "pool"))
@pytest.mark.parametrize("name", ["pass", "repack_every"])
def test_stack_spill_across_launches(P, pto, renderer, name, pipeline, flags):
    """The stacked glass layers spill every ray's traversal stack past the 12 LDS entries into the overflow columns, which are indexed by
    queue entry: one vertex per launch, and with re-packs that move the entries between launches, the frame stays the oracle's."""
    sd = adv.stacked_layers(W, H)
    r = sc.tuned(P, name, W, H)
    try:
        for layout in (2, 68):
            params = P.make_params(W, H, flags=flags, **FRAMES["k4"])
            r.SetScene(sd, layout)
            check_against_oracle(P, pto, r, sd, (name, pipeline, layout), params)
            assert r.BvhInfo().stack_need > 12
            r.Params = params
            st = r.Render(0.0)
            sc.check_stats(name, st, default_stats(renderer, sd, layout, params, ("layers", pipeline, layout)), live_slots(params),
                           (pipeline, layout))
    finally:
        r.Dispose()
