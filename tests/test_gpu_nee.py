"""-m gpu: next-event estimation (PT_FLAG_NEXT_EVENT, docs/SPEC.md §7) on the device against the scalar checker of tests/nee_ref/.

Every frame is compared bit for bit, with `rays` equal to the checker's extension plus shadow rays, over the synthetic scenes, a scene
of many lights of different sizes and emissions, every BVH layout and both builders, several stream counts and path depths. Also:
progressive frames, multi-rank frames, geometry updates (host and device memory), and the pipelines that refuse NEE."""
import numpy as np
import pytest

import nee_checker as nc
from frame_checks import check_nee as check
from frame_checks import nee_params
from pipelines import refused
from trace_support import H, LAYOUTS, W

pytestmark = pytest.mark.gpu


def scenes(P):
    N = P.native
    return {
        "cornell": P.make_scene(N.PT_SCENE_CORNELL, 0, 3, W, H),
        "glass": P.make_scene(N.PT_SCENE_CORNELL_GLASS, 0, 3, W, H),
        "tess": P.make_scene(N.PT_SCENE_CORNELL_TESS, 2000, 3, W, H),
        "lights": nc.many_lights_scene(P, W, H),
        "grazing": nc.grazing_scene(P, W, H),
    }


@pytest.mark.parametrize("name", ["cornell", "glass", "lights", "grazing"])
def test_layouts_and_builders(P, pto, renderer, name):
    """Every layout, both builders: the checker's frame and ray count."""
    N = P.native
    sd = scenes(P)[name]
    params = nee_params(P, spp=4, max_depth=8, streams=2)
    for width in LAYOUTS:
        for build in (0, N.PT_BVH_BUILD_LBVH):
            renderer.SetScene(sd, width | build)
            renderer.Params = params
            st, cst = check(P, pto, renderer, sd, params, (name, width, build))
            assert cst.shadow_rays > 0 and cst.n_lights > 0


def test_tessellated_bvh4q(P, pto, renderer):
    """A reduced C5 (tessellated walls) on the default BVH4Q, both builders."""
    N = P.native
    sd = scenes(P)["tess"]
    params = nee_params(P, spp=4, max_depth=8, streams=4)
    for build in (0, N.PT_BVH_BUILD_LBVH):
        renderer.SetScene(sd, N.PT_BVH_WIDTH_4Q | build)
        renderer.Params = params
        check(P, pto, renderer, sd, params, build)


@pytest.mark.parametrize("streams", [1, 8])
@pytest.mark.parametrize("depth", [1, 2, 8])
def test_streams_and_depths(P, pto, renderer, streams, depth):
    sd = scenes(P)["lights"]
    renderer.SetScene(sd, 0)
    params = nee_params(P, spp=8, max_depth=depth, streams=streams)
    renderer.Params = params
    st, cst = check(P, pto, renderer, sd, params, (streams, depth))
    if depth == 1:
        assert cst.shadow_rays == 0  # no vertex below max_depth: the plain frame


def test_extension_rays_are_the_plain_frame(P, pto, renderer):
    """The BSDF-sampled paths do not depend on NEE: rays(NEE) - rays(plain) = the checker's shadow rays, on every scene; and a scene
    without emissive triangles (C3 soup, sky-lit) renders the plain frame bit for bit."""
    N = P.native
    for name, sd in list(scenes(P).items()) + [("soup", P.make_scene(N.PT_SCENE_TRIANGLE_SOUP, 500, 3, W, H))]:
        renderer.SetScene(sd, 0)
        renderer.Params = P.make_params(W, H, spp=4, max_depth=8, streams=2)
        plain = renderer.Render(0.0)
        plain_img = renderer.ReadFramebuffer()
        renderer.Params = nee_params(P, spp=4, max_depth=8, streams=2)
        st, cst = check(P, pto, renderer, sd, renderer.Params, name)
        assert plain.rays == cst.ext_rays, name
        if name == "soup":
            assert cst.n_lights == 0 and st.rays == plain.rays
            assert np.array_equal(renderer.ReadFramebuffer(), plain_img)


def test_progressive(P, pto, renderer):
    """Four accumulate calls of 4 spp = one call of 16 spp; NEE and plain sums do not mix."""
    N = P.native
    sd = scenes(P)["lights"]
    renderer.SetScene(sd, 0)
    renderer.Params = nee_params(P, spp=16, max_depth=8, streams=4)
    whole = renderer.Render(0.0)
    want = renderer.ReadFramebuffer()
    rays = 0
    for k in range(4):
        p = nee_params(P, spp=4, max_depth=8, streams=4, sample_offset=4 * k)
        if k:
            p.flags |= N.PT_FLAG_ACCUMULATE
        renderer.Params = p
        rays += renderer.Render(0.0).rays
    assert np.array_equal(renderer.ReadFramebuffer(), want) and rays == whole.rays
    p = P.make_params(W, H, spp=4, max_depth=8, streams=4, sample_offset=16, flags=N.PT_FLAG_ACCUMULATE)
    renderer.Params = p
    with pytest.raises(P.PtException, match="NEXT_EVENT"):
        renderer.Render(0.0)
    renderer.Params = P.make_params(W, H, spp=4, max_depth=8, streams=4)  # plain sums ...
    renderer.Render(0.0)
    p = nee_params(P, spp=4, max_depth=8, streams=4, sample_offset=4)
    p.flags |= N.PT_FLAG_ACCUMULATE
    renderer.Params = p
    with pytest.raises(P.PtException, match="NEXT_EVENT"):  # ... are not continued by NEE
        renderer.Render(0.0)


def test_multi_rank(P, pto, renderer):
    """Three virtual ranks on one context assemble the single-rank frame; their rays add up."""
    sd = scenes(P)["lights"]
    renderer.SetScene(sd, 0)
    params = nee_params(P, spp=4, max_depth=8, streams=2)
    renderer.Params = params
    one = renderer.Render(0.0)
    want = renderer.ReadFramebuffer()
    with P.Comm([renderer] * 3, root=2) as comm:
        stats = comm.Render(nee_params(P, spp=4, max_depth=8, streams=2))
        assert sum(s.rays for s in stats) == one.rays and sum(s.paths for s in stats) == one.paths
        assert np.array_equal(renderer.ReadFramebuffer(), want)


def test_updates_move_the_lights(P, pto, renderer):
    """After pt_scene_update_triangles moves the light quad (and resizes it), from host and from device memory, a NEE frame equals
    the frame of a fresh commit of the moved geometry, and the checker's."""
    import dataclasses
    import torch
    N = P.native
    sd = scenes(P)["cornell"]
    light = np.nonzero(sd.mats["emission"].sum(axis=1)[sd.tri_mat] > 0)[0]
    v2 = sd.verts.copy()
    q = v2[light].reshape(-1, 3, 3)
    q[:, :, 0] = q[:, :, 0] * 1.5 + 0.2   # wider, off centre
    q[:, :, 1] -= 0.3                      # lower
    v2[light] = q.reshape(-1, 9)
    moved = dataclasses.replace(sd, verts=v2)
    params = nee_params(P, spp=4, max_depth=8, streams=2)
    for width in (2, 68, 73):
        for build in (0, N.PT_BVH_BUILD_LBVH):
            renderer.SetScene(moved, width | build)
            renderer.Params = params
            renderer.Render(0.0)
            fresh = renderer.ReadFramebuffer()
            for verts in (v2, torch.from_numpy(v2).cuda()):
                renderer.SetScene(sd, width | build)
                renderer.UpdateGeometry(verts=verts)
                renderer.Params = params
                check(P, pto, renderer, moved, params, (width, build, type(verts)))
                assert np.array_equal(renderer.ReadFramebuffer(), fresh), (width, build, type(verts))


def test_refused_pipelines(P, pto, renderer):
    """Packed, pooled, split and bucket pipelines, a forced extend_kernel 2 / 3 and visit counting refuse NEE with
    PT_ERR_UNSUPPORTED, and the context renders the next frame correctly."""
    N = P.native
    sd = scenes(P)["cornell"]
    renderer.SetScene(sd, 0)
    for flags in [r.flags for r in refused("nee")]:
        p = nee_params(P, spp=2, max_depth=8)
        p.flags |= flags
        renderer.Params = p
        with pytest.raises(P.PtException) as e:
            renderer.Render(0.0)
        assert e.value.status == N.PT_ERR_UNSUPPORTED, flags
    tuning = renderer.GetTuning().extend_kernel
    try:
        for k in [r.tuned_kernel for r in refused("nee", tuned=True)]:
            renderer.SetTuning(extend_kernel=k)
            renderer.Params = nee_params(P, spp=2, max_depth=8)
            with pytest.raises(P.PtException) as e:
                renderer.Render(0.0)
            assert e.value.status == N.PT_ERR_UNSUPPORTED, k
    finally:
        renderer.SetTuning(extend_kernel=tuning)
    p = nee_params(P, spp=4, max_depth=8, streams=2)
    p.flags |= N.PT_FLAG_EXTEND_SIMPLE | N.PT_FLAG_PROFILE_KERNELS  # the kernel NEE runs on, forced, and timed: accepted
    renderer.Params = p
    check(P, pto, renderer, sd, p, "after refusals")


def test_destroyed_contexts_and_scenes_return_their_device_memory(P):
    """Object lifetimes: a destroyed context gives back its NEE frame state (nee_ext + nee_rad, 32 bytes per path slot) and a destroyed
    scene its light table (lights, CDF and the per-triangle pa array, 4 bytes per blob triangle). Free device memory is read from
    torch.cuda.mem_get_info(). Both bounds are half of what the leak they guard against would take, derived from those sizes:
      context leg: six create / 1080p NEE frame (8 streams) / destroy cycles after a warm-up cycle may cost at most half of ONE cycle's
                   nee_ext + nee_rad = 510 tiles x 4096 pixels x 8 streams x 32 B / 2 = 267 MB (leaking them costs six times 535 MB);
      scene leg:   32 commits of the 1M-triangle tessellated Cornell box (LBVH) on one Renderer, then a small scene, may cost at most
                   half of 32 x 4 B x blob triangles = 67 MB (leaking pa alone costs 134 MB).
    Two idle readings a second apart are printed first: the device is shared, and a drift of that size would be the machine's."""
    import time
    import torch
    N = P.native
    w, h = 1920, 1080

    def free_bytes():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    cornell = P.make_scene(N.PT_SCENE_CORNELL, 0, 3, w, h)
    params = P.make_params(w, h, spp=8, max_depth=8, streams=8, flags=N.PT_FLAG_NEXT_EVENT)
    lay = P.tile_layout(params)
    assert lay.tiles_per_rank == 510

    def cycle():
        with P.Renderer(P.Window(w, h)) as r:
            r.Init()
            r.SetScene(cornell, 0)
            r.Params = params
            assert r.Render(0.0).rays > 0

    idle = free_bytes()
    time.sleep(1.0)
    print(f"\nidle drift over 1 s: {idle - free_bytes()} B")
    cycle()  # warm-up: the runtime's own one-time allocations
    before = free_bytes()
    for _ in range(6):
        cycle()
    ctx_drop, ctx_limit = before - free_bytes(), lay.tiles_per_rank * 4096 * 8 * 32 // 2
    print(f"context leg: free memory dropped by {ctx_drop} B over six cycles (limit {ctx_limit} B)")

    tess = P.make_scene(N.PT_SCENE_CORNELL_TESS, 1 << 20, 3, w, h)
    with P.Renderer(P.Window(w, h)) as r:
        r.Init()
        r.SetScene(tess, N.PT_BVH_BUILD_LBVH)  # warm-up (the builder's code objects), left the way the measured run ends
        n_blob = r.BvhInfo().n_tris
        assert n_blob > 1000000
        r.SetScene(cornell, 0)
        before = free_bytes()
        for _ in range(32):
            r.SetScene(tess, N.PT_BVH_BUILD_LBVH)
        r.SetScene(cornell, 0)  # destroys the last big scene
        scene_drop, scene_limit = before - free_bytes(), 32 * 4 * n_blob // 2
        print(f"scene leg: free memory dropped by {scene_drop} B over 32 commits of {n_blob} triangles (limit {scene_limit} B)")
    assert ctx_drop <= ctx_limit, ("context leg", ctx_drop, ctx_limit)  # (both legs are measured before either is judged)
    assert scene_drop <= scene_limit, ("scene leg", scene_drop, scene_limit)
