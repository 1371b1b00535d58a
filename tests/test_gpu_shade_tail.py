"""-m gpu: the end of shade_one (kernels.hip) against the oracle, bit for bit.

A path vertex ends in one of two ways: the path goes on (a BSDF sample gives the next ray) or it ends (sky, max_depth, zero
throughput, Russian roulette) and the slot's stream regenerates its next camera ray in place, if it has one. shade_one decides which
first, and then the Lambert vertices that go on and the regenerated camera rays draw their two random numbers and normalize their
direction in ONE pass: dimensions (4 + 4b, 5 + 4b) of the old key for the one kind, (0, 1) of the new key for the other, 0.5 by a
select without jitter. What can go wrong is the (key, dimension) a lane draws from, the vector it normalizes, the state it keeps
(origin, throughput, depth, sample) and the lanes that take neither way (streams that have run dry, metal and glass vertices).

64x48 frames, so that every wave is a mix of both kinds from the second vertex on:
  box    : a closed Lambert room with two Lambert spheres and a light — paths go on until roulette or max_depth ends them
  open   : a floor and three spheres under a bright sky — most vertices end the path and regenerate
  palette: tests/material_zoo.py's soup of 320 materials of all three kinds
with jitter on and off, spp in {1, 3, 8, 13} against streams in {1, 4, 8} (streams run dry in the middle of a launch, and some never
start), max_depth in {1, 2, 8}, rr_start in {0, 3}, every shading pipeline, progressive frames and next-event estimation."""
import numpy as np
import pytest

import material_zoo as mz
import nee_checker as nc
from frame_checks import check_nee
from pipelines import named_flags

pytestmark = pytest.mark.gpu

W, H = mz.W, mz.H
SPP = (1, 3, 8, 13)
STREAMS = (1, 4, 8)
DEPTH_RR = ((1, 0), (2, 3), (8, 0), (8, 3))  # (max_depth, rr_start): every max_depth and every rr_start of the grid


def box():
    mats = [mz.mat(mz.LAMBERT, (0.75, 0.75, 0.75)), mz.mat(mz.LAMBERT, (0.8, 0.2, 0.2)), mz.mat(mz.LAMBERT, (0.2, 0.8, 0.2)),
            mz.mat(mz.LAMBERT, (0.0, 0.0, 0.0), emission=(14.0, 12.0, 9.0)), mz.mat(mz.LAMBERT, (0.9, 0.9, 0.3)),
            mz.mat(mz.LAMBERT, (0.0, 0.0, 0.0))]  # 5: a black sphere: T * albedo == 0 ends the path
    faces = [((-1, -1, 1), (0, 2, 0), (2, 0, 0), 0), ((1, -1, -1), (0, 2, 0), (-2, 0, 0), 0),   # z = +1, z = -1, facing inwards
             ((1, -1, 1), (0, 2, 0), (0, 0, -2), 2), ((-1, -1, -1), (0, 2, 0), (0, 0, 2), 1),   # x = +1, x = -1
             ((-1, 1, 1), (0, 0, -2), (2, 0, 0), 0), ((-1, -1, -1), (0, 0, 2), (2, 0, 0), 0)]   # y = +1, y = -1
    tris, tm = [], []
    for p0, eu, ev, m in faces:
        tris += mz.quad(p0, eu, ev); tm += [m, m]
    tris += mz.quad((-0.4, 0.995, 0.4), (0, 0, -0.8), (0.8, 0, 0)); tm += [3, 3]                # the light under the ceiling
    spheres = [(-0.4, -0.65, -0.3, 0.35), (0.45, -0.75, 0.2, 0.25), (0.0, 0.1, -0.6, 0.2)]
    cam = mz.camera((0.0, 0.0, 0.95), (0.0, -0.1, -1.0), fov_deg=70)
    return mz.scene(tris, tm, spheres, [4, 0, 5], mats, cam, (0.0, 0.0, 0.0))


def open_air():
    mats = [mz.mat(mz.LAMBERT, (0.6, 0.6, 0.6)), mz.mat(mz.LAMBERT, (0.9, 0.4, 0.2)), mz.mat(mz.LAMBERT, (0.2, 0.4, 0.9)),
            mz.mat(mz.LAMBERT, (0.5, 0.5, 0.5), emission=(0.5, 0.5, 0.5))]
    tris = mz.quad((-3, -0.5, -3), (0, 0, 6), (6, 0, 0))
    spheres = [(-0.7, 0.0, 0.0, 0.5), (0.6, -0.1, 0.3, 0.4), (0.1, 0.9, -0.5, 0.3)]
    cam = mz.camera((0.0, 1.2, 4.0), (0.0, 0.1, 0.0), fov_deg=60)
    return mz.scene(tris, [0, 0], spheres, [1, 2, 3], mats, cam, (1.0, 0.9, 0.8))


SCENES = {"box": box, "open": open_air, "palette": lambda: mz.build("palette", "front")}


def pipelines(P):
    return named_flags("simple", "probed", "packed", "split", "bucket", "pool")


def frame(P, r, params):
    r.Params = params
    st = r.Render(0.0)
    return r.ReadFramebuffer(), st


def equal(P, pto, r, osc, kw, flags, count, ctx):
    N = P.native
    ref, ost = pto.render(osc, P.make_params(W, H, **kw))
    img, st = frame(P, r, P.make_params(W, H, flags=flags | (N.PT_FLAG_COUNT_VISITS if count else 0), **kw))
    assert np.array_equal(img, ref), (ctx, int((img != ref).any(axis=2).sum()))
    assert (st.rays, st.paths) == (ost.rays, ost.paths), (ctx, st.rays, ost.rays)
    if count:
        assert (st.node_visits, st.tri_tests, st.sphere_tests) == (ost.node_visits, ost.tri_tests, ost.sphere_tests), ctx
    return ost


@pytest.mark.parametrize("jitter", [1, 0], ids=["jitter", "centre"])
@pytest.mark.parametrize("name", list(SCENES))
def test_frames_equal_the_oracle(P, pto, renderer, name, jitter):
    """The grid of spp, streams, max_depth and rr_start. Every combination runs on the one-ray-per-lane kernel, and on one more
    pipeline in turn; the visit counters are compared on every second frame."""
    sd = SCENES[name]()
    sd.cam.jitter = jitter
    k = 0
    for li, layout in enumerate((0, 68)):  # the grid is dealt over the two layouts like a checkerboard: each sees every value of every axis
        renderer.SetScene(sd, layout)
        osc = pto.Scene(sd, (renderer.BvhInfo().width,) + renderer.BvhRead())
        for a, spp in enumerate(SPP):
            for b, streams in enumerate(STREAMS):
                for c, (max_depth, rr_start) in enumerate(DEPTH_RR):
                    if (a + b + c) % 2 != li:
                        continue
                    kw = dict(spp=spp, streams=streams, max_depth=max_depth, rr_start=rr_start)
                    pipes = pipelines(P)
                    for pname, flags in (pipes[0], pipes[1 + (k // 2) % (len(pipes) - 1)]):
                        ost = equal(P, pto, renderer, osc, kw, flags, (k // 2 + k) % 2 == 1, (name, jitter, layout, kw, pname))
                        k += 1
                    if max_depth == 1:
                        assert ost.rays == W * H * spp
    assert k == 2 * len(SPP) * len(STREAMS) * len(DEPTH_RR)


@pytest.mark.parametrize("name", list(SCENES))
def test_every_pipeline(P, pto, renderer, name):
    """One frame whose streams run dry at different vertices (13 samples over 4 streams) through each pipeline, with counters."""
    sd = SCENES[name]()
    sd.cam.jitter = 1
    renderer.SetScene(sd, 0)
    osc = pto.Scene(sd, (renderer.BvhInfo().width,) + renderer.BvhRead())
    for pname, flags in pipelines(P):
        for count in (False, True):
            equal(P, pto, renderer, osc, dict(spp=13, streams=4, max_depth=8, rr_start=3), flags, count, (name, pname, count))


@pytest.mark.parametrize("name", list(SCENES))
def test_progressive_frames(P, pto, renderer, name):
    """PT_FLAG_ACCUMULATE in two calls (5 + 8 samples over 4 streams: the second call starts in the middle of the stream rotation) is
    the oracle's 13-sample frame."""
    N = P.native
    sd = SCENES[name]()
    sd.cam.jitter = 1
    renderer.SetScene(sd, 0)
    osc = pto.Scene(sd, (renderer.BvhInfo().width,) + renderer.BvhRead())
    ref, _ = pto.render(osc, P.make_params(W, H, spp=13, max_depth=8, rr_start=3, streams=4))
    for pname, flags in pipelines(P)[:3]:
        frame(P, renderer, P.make_params(W, H, spp=5, max_depth=8, rr_start=3, streams=4, flags=flags))
        img, _ = frame(P, renderer, P.make_params(W, H, spp=8, max_depth=8, rr_start=3, streams=4, sample_offset=5,
                                                  flags=flags | N.PT_FLAG_ACCUMULATE))
        assert np.array_equal(img, ref), (name, pname)


@pytest.mark.parametrize("name", ["box", "palette"])
def test_next_event_estimation(P, pto, renderer, name):
    """PT_FLAG_NEXT_EVENT keeps the two-branch end (its light sample sits between the BSDF sample and the regeneration) and shares
    sample_lambert's and camera_ray's split forms: bit for bit the scalar checker of docs/SPEC.md §7 (pto.render has no light
    sampling; tests/nee_ref is the reference of every NEE test), rays and paths equal."""
    nc.build()
    sd = SCENES[name]()
    for jitter in (1, 0):
        sd.cam.jitter = jitter
        for layout in (0, 68):
            renderer.SetScene(sd, layout)
            for spp, streams, max_depth, rr_start in ((13, 4, 8, 3), (3, 8, 2, 0), (8, 1, 8, 0)):
                params = P.make_params(W, H, spp=spp, streams=streams, max_depth=max_depth, rr_start=rr_start, flags=P.native.PT_FLAG_NEXT_EVENT)
                renderer.Params = params
                _, cst = check_nee(P, pto, renderer, sd, params, (name, jitter, layout, spp, streams, max_depth, rr_start))
                assert cst.shadow_rays > 0
