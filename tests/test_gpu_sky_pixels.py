"""-m gpu: pixels that provably see only the sky are resolved at frame start instead of being traced (frame.cpp scene_pixels, kernels.hip
k_sky_pixels). Nothing about a frame may change: every frame here is compared with the oracle's on the same scene, BVH bytes and
parameters, bit for bit, and so is its ray count. A wrongly resolved pixel is a differing pixel, so the frames have their silhouettes
next to the bound: the boxes of the generator scenes fill their own bounding rectangle, spheres touch it, cameras are turned.

Before a frame is relied on, the oracle alone says that it has both kinds of pixel (has_both): a pixel whose every sample missed shows
exactly the value of the same frame of an empty scene.

test_sky_frame_needs_no_launches shows that the shortcut acts at all: a frame whose scene is wholly off-screen ends within the host's
run-ahead instead of after spp / bounces launches."""
import dataclasses

import numpy as np
import pytest

import env_checker as ec
from camera_space import SKY, empty_like, scene_of, spheres_only, turned
from frame_checks import check_nee, run_both
from pipelines import flags_of

pytestmark = pytest.mark.gpu


def has_both(P, pto, sd, params, ref):
    """Per the oracle: some pixels of `ref` saw nothing but sky in every sample, and some saw the scene."""
    void, _ = pto.render(pto.Scene(empty_like(P, sd)), params)
    sky = (ref == void).all(axis=2)
    return 0.02 < sky.mean() < 0.98


def exact(P, pto, r, sd, params, width=0, both=True):
    img, st, ref, ost = run_both(P, pto, r, sd, params, width)
    if both:
        assert has_both(P, pto, sd, params, ref), "the frame must have sky pixels and scene pixels"
    bad = np.argwhere((img != ref).any(axis=2))
    assert len(bad) == 0, (len(bad), bad[:4].tolist(), img[tuple(bad[0])].tolist(), ref[tuple(bad[0])].tolist())
    assert (st.rays, st.paths) == (ost.rays, ost.paths), (st.rays, ost.rays, st.paths, ost.paths)
    return img, st, ref, ost


@pytest.mark.parametrize("kind", ["PT_SCENE_CORNELL", "PT_SCENE_CORNELL_GLASS", "PT_SCENE_CORNELL_TESS"])
@pytest.mark.parametrize("w,h", [(200, 150), (100, 37)])
def test_generator_scenes(P, pto, renderer, kind, w, h):
    """The default camera: 7 samples over 4 streams, and 3 over 8 (streams without a sample: the dense frame start)."""
    sd = scene_of(P, kind, w, h)
    exact(P, pto, renderer, sd, P.make_params(w, h, spp=7, max_depth=8, streams=4))
    exact(P, pto, renderer, sd, P.make_params(w, h, spp=3, max_depth=8, streams=8))


@pytest.mark.parametrize("width", [2, 4, 68, 72, 73])
def test_layouts_builders_and_turned_cameras(P, pto, renderer, width):
    """The root's boxes are read in every node layout, from both builders; the camera's basis is not the world's."""
    N = P.native
    sd = scene_of(P, "PT_SCENE_CORNELL_TESS", 256, 160)
    for build, yaw, shift in ((0, 0.3, (1.0, 0.0, 0.0)), (N.PT_BVH_BUILD_LBVH, -0.2, (-0.6, 0.3, 1.0))):
        exact(P, pto, renderer, turned(sd, yaw, shift), P.make_params(256, 160, spp=5, max_depth=6, streams=2), width | build)


def test_progressive_accumulation(P, pto, renderer):
    """Calls of 3 + 5 + 2 samples continue the partial sums of the sky pixels bit for bit."""
    N = P.native
    sd = scene_of(P, "PT_SCENE_CORNELL_GLASS", 200, 150)
    renderer.SetScene(sd, 0)
    for streams in (1, 4):
        done, rays = 0, 0
        for n in (3, 5, 2):
            renderer.Params = P.make_params(200, 150, spp=n, max_depth=8, streams=streams, sample_offset=done,
                                            flags=N.PT_FLAG_ACCUMULATE if done else 0)
            rays += renderer.Render(0.0).rays
            done += n
        img = renderer.ReadFramebuffer()
        info = renderer.BvhInfo()
        whole = P.make_params(200, 150, spp=10, max_depth=8, streams=streams)
        ref, ost = pto.render(pto.Scene(sd, (info.width,) + renderer.BvhRead()), whole)
        assert has_both(P, pto, sd, whole, ref)
        assert np.array_equal(img, ref) and rays == ost.rays, (streams, rays, ost.rays)


def test_three_ranks(P, pto, renderer):
    """Every rank of three rendered and assembled: the tile partition still resolves the right slots."""
    sd = scene_of(P, "PT_SCENE_CORNELL", 200, 150)
    whole = P.make_params(200, 150, spp=5, max_depth=6, streams=2)
    _, _, ref, ost = exact(P, pto, renderer, sd, whole)
    with P.Comm([renderer] * 3, root=0) as comm:
        rays = 0
        for rank in range(3):
            renderer.Params = P.make_params(200, 150, spp=5, max_depth=6, streams=2, rank=rank, nranks=3)
            rays += renderer.Render(0.0).rays
            comm.StageTiles(rank)
        comm.Assemble(whole)
    assert rays == ost.rays and np.array_equal(renderer.ReadFramebuffer(), ref)


def test_both_kernels(P, pto, renderer):
    """The one-ray-per-lane and the lane-packing kernel agree with the oracle, and so with each other."""
    N = P.native
    for kind, w, h in (("PT_SCENE_CORNELL_TESS", 200, 150), ("PT_SCENE_CORNELL_GLASS", 100, 37)):
        sd = scene_of(P, kind, w, h)
        for flag in flags_of("simple", "packed"):
            for spp, streams in ((7, 4), (3, 8)):
                _, st, _, _ = exact(P, pto, renderer, sd, P.make_params(w, h, spp=spp, max_depth=8, streams=streams, flags=flag))
                assert st.reserved[0] == (2 if flag == N.PT_FLAG_EXTEND_PACKED else 1)


def test_spheres_only(P, pto, renderer):
    sd = spheres_only(P, 200, 150)
    exact(P, pto, renderer, sd, P.make_params(200, 150, spp=6, max_depth=5, streams=4))
    exact(P, pto, renderer, turned(spheres_only(P, 100, 37), 0.25), P.make_params(100, 37, spp=6, max_depth=5, streams=1))
    moved = np.array(sd.spheres)
    moved[:, 0] += 0.8  # pt_scene_update_spheres: the bound follows
    renderer.SetScene(sd, 0)
    renderer.UpdateGeometry(spheres=moved)
    p = P.make_params(200, 150, spp=4, max_depth=5, streams=2)
    renderer.Params = p
    st = renderer.Render(0.0)
    sd2 = dataclasses.replace(sd, spheres=moved)
    ref, ost = pto.render(pto.Scene(sd2), p)
    assert has_both(P, pto, sd2, p, ref)
    assert np.array_equal(renderer.ReadFramebuffer(), ref) and st.rays == ost.rays


def test_camera_inside_and_scene_behind(P, pto, renderer):
    """Nothing can be resolved with the camera inside the box, nor with a part of the scene behind the camera plane; the frames stay
    the oracle's."""
    sd = scene_of(P, "PT_SCENE_CORNELL", 200, 150)
    p = P.make_params(200, 150, spp=4, max_depth=6, streams=2)
    exact(P, pto, renderer, turned(sd, 0.0, (0.0, 0.0, -3.2)), p, both=False)      # inside
    exact(P, pto, renderer, turned(sd, 1.2, (0.0, 0.0, -2.2)), p, both=False)      # in front of the opening, turned aside
    exact(P, pto, renderer, turned(sd, 0.0, (0.0, 0.0, -5.5)), p, both=False)      # behind the box, looking away from it


def test_refit_moves_the_bound(P, pto, renderer):
    """pt_scene_update_triangles moves the scene into what was sky in the frame before: from host memory and from device memory, where
    the host never sees the vertices."""
    import torch
    sd = scene_of(P, "PT_SCENE_CORNELL_TESS", 256, 160)
    sd.cam.origin[2] += 2.0  # further away: room to move sideways inside the image
    p = P.make_params(256, 160, spp=4, max_depth=6, streams=2)
    for width in (0, 2):
        _, _, before, _ = exact(P, pto, renderer, sd, p, width)
        for k, dx in enumerate((1.1, -1.3)):
            moved = dataclasses.replace(sd, verts=(np.array(sd.verts).reshape(-1, 3, 3) + np.float32([dx, 0.2, 0.0])).reshape(-1, 9),
                                        spheres=np.array(sd.spheres) + np.float32([dx, 0.2, 0.0, 0.0]))
            renderer.UpdateGeometry(verts=torch.as_tensor(moved.verts, device="cuda") if k else moved.verts, spheres=moved.spheres)
            renderer.Params = p
            st = renderer.Render(0.0)
            info = renderer.BvhInfo()
            ref, ost = pto.render(pto.Scene(moved, (info.width,) + renderer.BvhRead()), p)
            void, _ = pto.render(pto.Scene(empty_like(P, sd)), p)
            was_sky, is_sky = (before == void).all(axis=2), (ref == void).all(axis=2)
            assert (was_sky & ~is_sky).mean() > 0.02 and is_sky.mean() > 0.02, "the scene must move into former sky"
            assert np.array_equal(renderer.ReadFramebuffer(), ref) and st.rays == ost.rays, (width, dx)


def test_count_visits_frames_keep_the_specs_visits(P, pto, renderer):
    N = P.native
    sd = scene_of(P, "PT_SCENE_CORNELL_TESS", 200, 150)
    for flag in flags_of("simple", "packed"):
        p = P.make_params(200, 150, spp=3, max_depth=6, streams=2, flags=flag)
        img, st, ref, ost = run_both(P, pto, renderer, sd, p, 0, count=True)
        assert has_both(P, pto, sd, p, ref) and np.array_equal(img, ref)
        assert (st.rays, st.node_visits, st.tri_tests, st.sphere_tests) == (ost.rays, ost.node_visits, ost.tri_tests, ost.sphere_tests)


def test_environment_map_frames(P, pto, renderer):
    """A miss under an environment map depends on its direction: such frames resolve nothing and equal the checker's, as before."""
    w, h = 100, 37
    sun = ec.sun_sky(P)
    sd = dataclasses.replace(ec.scene(P, "cornell", w, h), environment=sun, sky=SKY)
    renderer.SetScene(sd, 0)
    for nee in (0, P.native.PT_FLAG_NEXT_EVENT):
        p = P.make_params(w, h, spp=4, max_depth=6, streams=2, flags=nee)
        renderer.Params = p
        st = renderer.Render(0.0)
        ref, cst, _ = ec.render(pto, pto.Scene(sd), p, env=sun, flags=ec.NEE if nee else 0)
        assert np.array_equal(renderer.ReadFramebuffer(), ref) and st.rays == cst.ext_rays + cst.shadow_rays
    renderer.SetEnvironment(None)  # and with the map gone the same scene resolves its sky pixels again
    p = P.make_params(w, h, spp=4, max_depth=6, streams=2)
    renderer.Params = p
    st = renderer.Render(0.0)
    plain = dataclasses.replace(sd, environment=None)
    info = renderer.BvhInfo()
    ref, ost = pto.render(pto.Scene(plain, (info.width,) + renderer.BvhRead()), p)
    assert has_both(P, pto, plain, p, ref) and np.array_equal(renderer.ReadFramebuffer(), ref) and st.rays == ost.rays


def test_next_event_frames(P, pto, renderer):
    """PT_FLAG_NEXT_EVENT frames take the shortcut too (a camera ray's miss adds the sky with weight 1): the NEE checker's frame."""
    sd = scene_of(P, "PT_SCENE_CORNELL", 100, 37)
    renderer.SetScene(sd, 0)
    for spp, streams in ((5, 2), (3, 8)):
        p = P.make_params(100, 37, spp=spp, max_depth=6, streams=streams, flags=P.native.PT_FLAG_NEXT_EVENT)
        renderer.Params = p
        check_nee(P, pto, renderer, sd, p, (spp, streams))


def test_sky_frame_needs_no_launches(P, pto):
    """Every pixel is sky: the scene is in front of the camera plane and wholly beside the image. Traced, one stream of 64 samples at
    4 vertices per launch takes at least 16 launches with rays; resolved, no launch after the first has any, and the host notices
    after its run-ahead of `lag` launches."""
    w, h = 100, 37
    sd = scene_of(P, "PT_SCENE_CORNELL", w, h)
    sd = dataclasses.replace(sd, verts=(np.array(sd.verts).reshape(-1, 3, 3) + np.float32([40.0, 0.0, 0.0])).reshape(-1, 9),
                             spheres=np.array(sd.spheres) + np.float32([40.0, 0.0, 0.0, 0.0]))
    r = P.Renderer(P.Window(w, h))
    r.Init()
    try:
        r.SetTuning(finish_below=0)
        t = r.GetTuning()
        lag = t.lag or 3 + (1 if t.readback == 0 else 0)
        for flag in flags_of("simple", "packed"):
            p = P.make_params(w, h, spp=64, max_depth=8, streams=1, flags=flag)
            img, st, ref, ost = run_both(P, pto, r, sd, p, 0)
            void, _ = pto.render(pto.Scene(empty_like(P, sd)), p)
            assert np.array_equal(ref, void) and ost.rays == w * h * 64, "the oracle sees nothing but sky"
            assert np.array_equal(img, ref) and (st.rays, st.paths) == (ost.rays, ost.paths)
            assert st.iterations <= lag + 2 < 16, (st.iterations, lag)
    finally:
        r.Dispose()
