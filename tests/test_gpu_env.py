"""-m gpu: environment-map lighting (pt_scene_set_environment, docs/SPEC.md §11) on the device against the scalar checker of
tests/env_ref/.

Every frame is compared bit for bit, with `rays` equal to the checker's extension plus shadow rays: over the sun-lit soup, Cornell and
Cornell-glass under the same map, every BVH layout and both builders, plain and with PT_FLAG_NEXT_EVENT, several stream counts, path
depths and map sizes. Also: a map of distinct texels seen directly, constant and black maps against sky frames, removal, setting after
commit, geometry updates, progressive and multi-rank frames, the pipelines that refuse such scenes, and pt_denoise's guides."""
import dataclasses

import numpy as np
import pytest

import env_checker as ec
from pipelines import refused
from trace_support import H, LAYOUTS, W

pytestmark = pytest.mark.gpu


def params_of(P, nee, **kw):
    p = P.make_params(W, H, **kw)
    if nee:
        p.flags |= P.native.PT_FLAG_NEXT_EVENT
    return p


def check(P, pto, r, sd, env, params, ctx):
    """The renderer's frame of its current scene = the checker's frame of (sd, env) bit for bit; rays = extension + shadow rays."""
    nee = bool(params.flags & P.native.PT_FLAG_NEXT_EVENT)
    st = r.Render(0.0)
    img = r.ReadFramebuffer()
    ref, cst, _ = ec.render(pto, pto.Scene(sd), params, env=env, flags=ec.NEE if nee else 0)
    assert np.isfinite(img).all(), ctx
    bad = np.argwhere((img != ref).any(axis=2))
    assert len(bad) == 0, (ctx, len(bad), bad[:4].tolist(), img[tuple(bad[0])].tolist(), ref[tuple(bad[0])].tolist())
    assert st.rays == cst.ext_rays + cst.shadow_rays, (ctx, st.rays, cst.ext_rays, cst.shadow_rays)
    assert st.paths == cst.paths and st.reserved[0] == 1, (ctx, st.paths, cst.paths, st.reserved[0])
    return st, cst


@pytest.fixture(scope="module")
def sun(P):
    return ec.sun_sky(P)


@pytest.mark.parametrize("nee", [False, True], ids=["plain", "nee"])
@pytest.mark.parametrize("name", ["soup", "cornell", "glass"])
def test_layouts_and_builders(P, pto, renderer, sun, name, nee):
    """Every layout, both builders: the checker's frame and ray count. The soup has the map as its only light, the boxes both kinds."""
    N = P.native
    sd = dataclasses.replace(ec.scene(P, name, W, H), environment=sun)
    params = params_of(P, nee, spp=4, max_depth=8, streams=2)
    for width in LAYOUTS:
        for build in (0, N.PT_BVH_BUILD_LBVH):
            renderer.SetScene(sd, width | build)
            renderer.Params = params
            st, cst = check(P, pto, renderer, sd, sun, params, (name, width, build))
            assert cst.lit == 1 and (cst.shadow_rays > 0) == nee and (cst.n_lights > 0) == (name != "soup")


@pytest.mark.parametrize("streams", [1, 8])
@pytest.mark.parametrize("depth", [1, 2, 8])
def test_streams_and_depths(P, pto, renderer, sun, streams, depth):
    sd = dataclasses.replace(ec.scene(P, "cornell", W, H), environment=sun)
    renderer.SetScene(sd, 0)
    for nee in (False, True):
        params = params_of(P, nee, spp=8, max_depth=depth, streams=streams)
        renderer.Params = params
        st, cst = check(P, pto, renderer, sd, sun, params, (streams, depth, nee))
        if depth == 1:
            assert cst.shadow_rays == 0  # no vertex below max_depth


@pytest.mark.parametrize("n", [1, 2, 5, 64])
def test_map_sizes(P, pto, renderer, n):
    """One texel, the four quadrant texels, an odd size, and the size of the other tests: sun maps and maps of distinct texels."""
    sd = ec.scene(P, "cornell", W, H)
    renderer.SetScene(sd, 0)
    for env in (ec.sun_sky(P, n), ec.distinct(n)):
        renderer.SetEnvironment(env)
        assert renderer.EnvironmentInfo().n == n and renderer.EnvironmentInfo().device_bytes >= n * n * 20 + n * 4
        for nee in (False, True):
            params = params_of(P, nee, spp=4, max_depth=8, streams=2)
            renderer.Params = params
            check(P, pto, renderer, sd, env, params, (n, nee))


def test_distinct_texels_seen_directly(P, pto, renderer):
    """Every texel its own colour, under a jitter-free camera at the origin looking down -z at one small triangle: the camera rays
    look the map up across the lower half's fold lines (the image's centre column and row) and along the -z axis (its centre pixel)."""
    sd = ec.one_triangle_scene(P, W, H)
    renderer.SetScene(sd, 0)
    for n in (8, 64):
        env = ec.distinct(n)
        renderer.SetEnvironment(env)
        for nee in (False, True):
            params = params_of(P, nee, spp=2, max_depth=4, streams=1)
            renderer.Params = params
            st, cst = check(P, pto, renderer, sd, env, params, (n, nee))
            assert cst.ext_rays > cst.paths  # the triangle is seen
        img = renderer.ReadFramebuffer()
        assert np.array_equal(img[H // 2, W // 2, :3], env[n - 1, n - 1])  # d = (+0, +0, -1): the corner u = v = 1
        assert len(np.unique(img[..., :3].reshape(-1, 3), axis=0)) > (40 if n == 64 else 20)  # many texels


def test_extension_rays_are_the_plain_frame(P, pto, renderer, sun):
    """rays(NEE) - rays(plain) = the checker's shadow rays, and the extension rays are the plain environment frame's."""
    for name in ("soup", "cornell", "glass"):
        sd = dataclasses.replace(ec.scene(P, name, W, H), environment=sun)
        renderer.SetScene(sd, 0)
        renderer.Params = params_of(P, False, spp=4, max_depth=8, streams=2)
        plain = renderer.Render(0.0)
        renderer.Params = params_of(P, True, spp=4, max_depth=8, streams=2)
        st, cst = check(P, pto, renderer, sd, sun, renderer.Params, name)
        assert plain.rays == cst.ext_rays and st.rays - plain.rays == cst.shadow_rays > 0, name


def test_constant_and_black_environments_are_sky_frames(P, pto, renderer):
    """A constant map = the same scene's `sky` frame from the default kernel (no environment: today's path), bit for bit; an all-black
    map, plain and with NEE, = the sky = 0 frames."""
    c = np.array([0.7, 0.9, 1.3], np.float32)
    for name in ("soup", "cornell", "glass"):
        base = ec.scene(P, name, W, H)
        for colour, env in ((c, np.full((5, 5, 3), c, np.float32)), (np.zeros(3, np.float32), np.zeros((4, 4, 3), np.float32))):
            sd = dataclasses.replace(base, sky=colour)
            for nee in (False, True):
                if nee and colour.any():
                    continue  # a constant map is a light and the sky is not: only the plain frames agree
                renderer.SetScene(sd, 0)
                renderer.Params = params_of(P, nee, spp=4, max_depth=8, streams=2)
                want_st = renderer.Render(0.0)
                want = renderer.ReadFramebuffer()
                renderer.SetEnvironment(env)
                got_st = renderer.Render(0.0)
                assert np.array_equal(renderer.ReadFramebuffer(), want), (name, nee, colour.tolist())
                assert got_st.rays == want_st.rays and got_st.reserved[0] == 1


def test_removal_after_commit_and_updates(P, pto, renderer, sun):
    """Set after commit: no new commit needed. A refused call keeps the map. It survives pt_scene_update_triangles. Removing it
    restores the earlier frames bit for bit."""
    sd = ec.scene(P, "cornell", W, H)
    renderer.SetScene(sd, 0)
    before = {}
    for nee in (False, True):
        renderer.Params = params_of(P, nee, spp=4, max_depth=8, streams=2)
        renderer.Render(0.0)
        before[nee] = renderer.ReadFramebuffer()
    assert renderer.EnvironmentInfo().n == 0
    renderer.SetEnvironment(sun)
    with pytest.raises(P.PtException):
        renderer.SetEnvironment(np.full((4, 4, 3), -1.0, np.float32))
    info = renderer.EnvironmentInfo()
    assert (info.n, info.lit) == (64, 1) and info.device_bytes >= 64 * 64 * 20 + 64 * 4
    for nee in (False, True):
        renderer.Params = params_of(P, nee, spp=4, max_depth=8, streams=2)
        check(P, pto, renderer, sd, sun, renderer.Params, ("after commit", nee))
    v2 = sd.verts.copy()
    v2[:, 1::3] *= 0.9  # squash the box
    renderer.UpdateGeometry(verts=v2)
    moved = dataclasses.replace(sd, verts=v2)
    for nee in (False, True):
        renderer.Params = params_of(P, nee, spp=4, max_depth=8, streams=2)
        check(P, pto, renderer, moved, sun, renderer.Params, ("after update", nee))
    renderer.UpdateGeometry(verts=sd.verts)
    renderer.SetEnvironment(None)
    assert renderer.EnvironmentInfo().n == 0
    for nee in (False, True):
        renderer.Params = params_of(P, nee, spp=4, max_depth=8, streams=2)
        renderer.Render(0.0)
        assert np.array_equal(renderer.ReadFramebuffer(), before[nee]), nee


def test_progressive(P, pto, renderer, sun):
    """Four accumulate calls of 4 spp = one call of 16 spp."""
    N = P.native
    sd = dataclasses.replace(ec.scene(P, "cornell", W, H), environment=sun)
    renderer.SetScene(sd, 0)
    for nee in (False, True):
        renderer.Params = params_of(P, nee, spp=16, max_depth=8, streams=4)
        whole, _ = check(P, pto, renderer, sd, sun, renderer.Params, ("whole", nee))
        want = renderer.ReadFramebuffer()
        rays = 0
        for k in range(4):
            p = params_of(P, nee, spp=4, max_depth=8, streams=4, sample_offset=4 * k)
            if k:
                p.flags |= N.PT_FLAG_ACCUMULATE
            renderer.Params = p
            rays += renderer.Render(0.0).rays
        assert np.array_equal(renderer.ReadFramebuffer(), want) and rays == whole.rays, nee


def test_multi_rank(P, pto, renderer, sun):
    """Three virtual ranks on one context assemble the single-rank frame; their rays add up."""
    sd = dataclasses.replace(ec.scene(P, "glass", W, H), environment=sun)
    renderer.SetScene(sd, 0)
    for nee in (False, True):
        renderer.Params = params_of(P, nee, spp=4, max_depth=8, streams=2)
        one = renderer.Render(0.0)
        want = renderer.ReadFramebuffer()
        with P.Comm([renderer] * 3, root=2) as comm:
            stats = comm.Render(params_of(P, nee, spp=4, max_depth=8, streams=2))
            assert sum(s.rays for s in stats) == one.rays and sum(s.paths for s in stats) == one.paths
            assert np.array_equal(renderer.ReadFramebuffer(), want), nee


def test_refused_pipelines(P, pto, renderer, sun):
    """Packed, pooled, split and bucket pipelines, visit counting and a forced extend_kernel 2 / 3 refuse a scene with an environment
    with PT_ERR_UNSUPPORTED and say why; the next ordinary frame is right."""
    N = P.native
    sd = dataclasses.replace(ec.scene(P, "cornell", W, H), environment=sun)
    renderer.SetScene(sd, 0)
    for nee in (False, True):
        for flags in [r.flags for r in refused("env")]:
            p = params_of(P, nee, spp=2, max_depth=8)
            p.flags |= flags
            renderer.Params = p
            with pytest.raises(P.PtException, match="environment") as e:
                renderer.Render(0.0)
            assert e.value.status == N.PT_ERR_UNSUPPORTED, flags
    tuning = renderer.GetTuning().extend_kernel
    try:
        for k in [r.tuned_kernel for r in refused("env", tuned=True)]:
            renderer.SetTuning(extend_kernel=k)
            renderer.Params = params_of(P, False, spp=2, max_depth=8)
            with pytest.raises(P.PtException, match="environment") as e:
                renderer.Render(0.0)
            assert e.value.status == N.PT_ERR_UNSUPPORTED, k
    finally:
        renderer.SetTuning(extend_kernel=tuning)
    for nee in (False, True):
        p = params_of(P, nee, spp=4, max_depth=8, streams=2)
        p.flags |= N.PT_FLAG_EXTEND_SIMPLE | N.PT_FLAG_PROFILE_KERNELS  # the kernel these frames run on, forced, and timed: accepted
        renderer.Params = p
        check(P, pto, renderer, sd, sun, p, ("after refusals", nee))


def test_denoise_guides_do_not_see_the_environment(P, pto, renderer, sun):
    """pt_denoise runs on an environment frame; its guides (a miss stays a miss) equal those of the scene without the map."""
    sd = ec.scene(P, "glass", W, H)
    renderer.SetScene(sd, 0)
    renderer.Params = params_of(P, False, spp=4, max_depth=8, streams=2)
    renderer.Render(0.0)
    renderer.Denoise(iterations=2)
    want = renderer.ReadGuides()
    renderer.SetEnvironment(sun)
    for nee in (False, True):
        renderer.Params = params_of(P, nee, spp=4, max_depth=8, streams=2)
        check(P, pto, renderer, sd, sun, renderer.Params, ("denoise", nee))
        st = renderer.Denoise(iterations=2)
        assert st.rays == W * H
        assert np.array_equal(renderer.ReadGuides().view(np.uint32), want.view(np.uint32))
        assert np.isfinite(renderer.ReadDenoised()).all()
