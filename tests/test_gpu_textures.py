"""-m gpu: albedo textures (docs/SPEC.md §13) on the device against the scalar checker of tests/tex_ref/.

Every frame is compared bit for bit, with `rays` and `paths` equal to the checker's and pt_stats.reserved[0] == 1 (the one-ray-per-lane
kernel): the Cornell box with all five walls textured and the soup with random UVs over every layout and both builders, plain, with
PT_FLAG_NEXT_EVENT, with an environment map and with both; every texture size and both filters; the glass box with a bound sphere
material; depths and streams; distinct texels seen directly; the invariants that need no checker; geometry updates, progressive and
multi-rank frames; pt_denoise's guides; and every refusal, after which the context still renders."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import env_checker as ec
import tex_checker as tc
from pipelines import FLAGS
from trace_support import H, LAYOUTS, W

pytestmark = pytest.mark.gpu

MODES = {"plain": (False, False), "nee": (True, False), "env": (False, True), "nee+env": (True, True)}
PT_ERR_UNSUPPORTED = 6


@pytest.fixture(scope="module")
def sun(P):
    return ec.sun_sky(P, 16)


def params_of(P, nee, **kw):
    p = P.make_params(W, H, **kw)
    if nee:
        p.flags |= P.native.PT_FLAG_NEXT_EVENT
    return p


def with_env(sd, env):
    return dataclasses.replace(sd, environment=env)


def reference(pto, sd, params, env, nee):
    """The checker's frame of the textured SceneData `sd` (computed once per case: it depends on neither layout nor builder)."""
    return tc.render(pto, pto.Scene(sd), params, sd, env=env, nee=nee)


def same_frame(P, r, ref, cst, ctx):
    """The renderer's frame of its current scene and Params = the checker's bit for bit; rays = extension + shadow rays; paths; kernel 1."""
    st = r.Render(0.0)
    img = r.ReadFramebuffer()
    assert np.isfinite(img).all(), ctx
    bad = np.argwhere((img.view(np.uint32) != ref.view(np.uint32)).any(axis=2))
    assert len(bad) == 0, (ctx, len(bad), bad[:4].tolist(), img[tuple(bad[0])].tolist(), ref[tuple(bad[0])].tolist())
    assert st.rays == cst.ext_rays + cst.shadow_rays, (ctx, st.rays, cst.ext_rays, cst.shadow_rays)
    assert st.paths == cst.paths and st.reserved[0] == 1, (ctx, st.paths, cst.paths, st.reserved[0])
    return st


def check(P, pto, r, sd, params, env, ctx):
    nee = bool(params.flags & P.native.PT_FLAG_NEXT_EVENT)
    ref, cst = reference(pto, sd, params, env, nee)
    r.Params = params
    return same_frame(P, r, ref, cst, ctx), cst


def two_textures(P, name):
    """The two scenes of the layout tests: two different textures, one bilinear and one nearest, bound in the Cornell box; the soup's one
    material with a bilinear 3 x 5."""
    if name == "cornell":
        return tc.cornell(P, W, H, tc.distinct(3, 5), (tc.distinct(2, 2, 40), tc.NEAREST))
    return dataclasses.replace(tc.soup(P, W, H, tc.distinct(3, 5)), sky=np.ones(3, np.float32))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["cornell", "soup"])
def test_layouts_and_builders(P, pto, renderer, sun, name, mode):
    N = P.native
    nee, has_env = MODES[mode]
    env = sun if has_env else None
    sd = with_env(two_textures(P, name), env)
    params = params_of(P, nee, spp=4, max_depth=8, streams=2)
    ref, cst = reference(pto, sd, params, env, nee)
    plain, _ = tc.render(pto, pto.Scene(sd), params, None, env=env, nee=nee)
    assert not np.array_equal(ref, plain)  # the textures are seen
    if name == "cornell":
        assert (cst.shadow_rays > 0) == nee
    for width in LAYOUTS:
        for build in (0, N.PT_BVH_BUILD_LBVH):
            renderer.SetScene(sd, width | build)
            renderer.Params = params
            same_frame(P, renderer, ref, cst, (name, mode, width, build))
            info = renderer.TextureInfo(0 if name == "cornell" else 1)
            assert (info.width, info.height, info.device_bytes) == (3, 5, 3 * 5 * 16) and info.materials == 1


@pytest.mark.parametrize("flags", [0, tc.NEAREST], ids=["bilinear", "nearest"])
@pytest.mark.parametrize("size", [(1, 1), (2, 2), (3, 5), (64, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_texture_sizes_and_filters(P, pto, renderer, sun, size, flags):
    """Every size with both filters on the white walls, a second texture with the other filter on the coloured walls."""
    sd = tc.cornell(P, W, H, (tc.distinct(*size), flags), (tc.distinct(5, 3, 11), flags ^ tc.NEAREST))
    renderer.SetScene(sd, 0)
    check(P, pto, renderer, sd, params_of(P, False, spp=4, max_depth=8, streams=2), None, (size, flags, "plain"))
    sde = with_env(sd, sun)
    renderer.SetEnvironment(sun)
    check(P, pto, renderer, sde, params_of(P, True, spp=4, max_depth=8, streams=2), sun, (size, flags, "nee+env"))


@pytest.mark.parametrize("mode", list(MODES))
def test_glass_box_with_a_bound_sphere_material(P, pto, renderer, sun, mode):
    """cornell_glass: textured walls, and the rough metal sphere's material bound too. The checker leaves spheres plain; the frame is its
    frame, and differs from the untextured one only through the walls."""
    nee, has_env = MODES[mode]
    env = sun if has_env else None
    sd = with_env(tc.cornell(P, W, H, tc.distinct(3, 5), (tc.distinct(2, 2, 40), tc.NEAREST), glass=True), env)
    assert sd.material_textures[5] == 3 and sd.mats[5]["kind"] == P.native.PT_METAL
    renderer.SetScene(sd, 0)
    params = params_of(P, nee, spp=4, max_depth=8, streams=2)
    check(P, pto, renderer, sd, params, env, ("glass", mode))
    only_walls = dataclasses.replace(sd, material_textures=np.where(np.arange(len(sd.mats)) == 5, tc.NO_TEXTURE, sd.material_textures).astype(np.uint32))
    ref, _ = reference(pto, only_walls, params, env, nee)
    assert np.array_equal(renderer.ReadFramebuffer().view(np.uint32), ref.view(np.uint32))  # the sphere stayed plain
    assert renderer.TextureInfo(3).materials == 3


@pytest.mark.parametrize("streams", [1, 8])
@pytest.mark.parametrize("depth", [1, 2, 8])
def test_depths_and_streams(P, pto, renderer, sun, depth, streams):
    sd = two_textures(P, "cornell")
    renderer.SetScene(sd, 0)
    for nee in (False, True):
        _, cst = check(P, pto, renderer, sd, params_of(P, nee, spp=8, max_depth=depth, streams=streams), None, (depth, streams, nee))
        if depth == 1:
            assert cst.shadow_rays == 0


def quad_scene(P, tex):
    """One quad of two triangles at z = -1 before a jitter-free camera at the origin, its material (albedo 0.5, 0.75, 0.25) bound to the
    nearest-filter texture `tex`, UVs spanning the texture about once and a half with a wrap. The sky is exactly 1: a path that leaves the
    quad carries T = albedo * texel to it, so at max_depth 2 a pixel of the quad is albedo * texel exactly, and with a black sky it is 0
    whatever the texture."""
    base = ec.one_triangle_scene(P, W, H)
    verts = np.array([[-2.5, -1.75, -1.0, 2.5, -1.75, -1.0, 2.5, 1.75, -1.0], [-2.5, -1.75, -1.0, 2.5, 1.75, -1.0, -2.5, 1.75, -1.0]], np.float32)
    uvs = np.array([[-0.25, 0.0, 1.25, 0.0, 1.25, 1.5], [-0.25, 0.0, 1.25, 1.5, -0.25, 1.5]], np.float32)
    mats = base.mats.copy()
    mats[0]["albedo"] = (0.5, 0.75, 0.25)
    sd = dataclasses.replace(base, verts=verts, tri_mat=np.zeros(2, np.uint32), mats=mats, sky=np.ones(3, np.float32))
    return tc.textured(sd, {2: (tex, tc.NEAREST)}, {0: 2}, uvs=uvs)


def jitter_free_rays(pto, cam):
    c = type(cam).from_buffer_copy(cam)
    c.jitter = 0
    o, d = np.empty((H * W, 3), np.float32), np.empty((H * W, 3), np.float32)
    for y in range(H):
        for x in range(W):
            o[y * W + x], d[y * W + x] = pto.camera_ray(c, x, y)
    return o, d


def test_distinct_texels_seen_directly(P, pto, renderer):
    tex = tc.distinct(7, 5)
    sd = quad_scene(P, tex)
    renderer.SetScene(sd, 0)
    renderer.Params = params_of(P, False, spp=1, max_depth=2, rr_start=8, streams=1)
    st = renderer.Render(0.0)
    img = renderer.ReadFramebuffer()
    assert st.reserved[0] == 1
    hits, _ = renderer.TraceRays(jitter_free_rays(pto, sd.cam))
    ids = np.ascontiguousarray(hits[:, 1]).view(np.uint32)
    alb = sd.mats[0]["albedo"].astype(np.float32)
    want = np.ones((H * W, 3), np.float32)
    for i in np.nonzero(ids != 0xFFFFFFFF)[0]:
        s, t = tc.coordinate(sd.uvs[ids[i]], hits[i, 2], hits[i, 3])
        want[i] = alb * tc.lookup(tex, s, t, tc.NEAREST)
    n_hit = int((ids != 0xFFFFFFFF).sum())
    assert 0.3 * W * H < n_hit < W * H
    assert np.array_equal(img[..., :3].reshape(-1, 3).view(np.uint32), want.view(np.uint32))
    assert len(np.unique(want[ids != 0xFFFFFFFF], axis=0)) == 35  # every texel of the 7 x 5 texture is seen
    # the whole frame against the checker as well, and the black sky
    check(P, pto, renderer, sd, renderer.Params, None, "quad")
    dark = dataclasses.replace(sd, sky=np.zeros(3, np.float32))
    renderer.SetScene(dark, 0)
    renderer.Render(0.0)
    assert not renderer.ReadFramebuffer()[..., :3].any()


def test_invariants_without_the_checker(P, pto, renderer):
    """All-ones textures give the untextured scene's frame bit for bit; removing the UVs or the binding and committing again restores it;
    the blob is the same with and without textures."""
    N = P.native
    plain = P.make_scene(N.PT_SCENE_CORNELL_GLASS, 0, 3, W, H)
    for width in (0, 68 | N.PT_BVH_BUILD_LBVH):
        renderer.SetScene(plain, width)
        blob = renderer.BvhRead()
        frames = {}
        for nee in (False, True):
            renderer.Params = params_of(P, nee, spp=4, max_depth=8, streams=2)
            frames[nee] = (renderer.Render(0.0).rays, renderer.ReadFramebuffer())
        for size, flags in (((1, 1), 0), ((3, 5), tc.NEAREST), ((64, 64), 0)):
            ones = (np.ones((size[1], size[0], 3), np.float32), flags)
            sd = tc.textured(plain, {0: ones, 63: ones}, {0: 0, 1: 63, 2: 63, 5: 0}, uvs=tc.random_uvs(len(plain.verts)))
            renderer.SetScene(sd, width)
            assert all(np.array_equal(a, b) for a, b in zip(renderer.BvhRead(), blob))
            for nee in (False, True):
                renderer.Params = params_of(P, nee, spp=4, max_depth=8, streams=2)
                st = renderer.Render(0.0)
                assert st.reserved[0] == 1 and st.rays == frames[nee][0], (size, nee)
                assert np.array_equal(renderer.ReadFramebuffer().view(np.uint32), frames[nee][1].view(np.uint32)), (size, flags, nee)
    sd = tc.cornell(P, W, H, tc.distinct(3, 5), tc.distinct(2, 2, 40), glass=True)
    for remove in ("uvs", "binding", "textures"):
        renderer.SetScene(sd, 0)
        renderer.Params = params_of(P, False, spp=4, max_depth=8, streams=2)
        renderer.Render(0.0)
        assert not np.array_equal(renderer.ReadFramebuffer(), frames[False][1])
        if remove == "uvs":
            renderer.SetTriangleUVs(None)
        elif remove == "binding":
            renderer.SetMaterialTextures(None)
        else:
            renderer.SetMaterialTextures(np.full(len(sd.mats), tc.NO_TEXTURE, np.uint32))
            renderer.SetTexture(0, None)
            renderer.SetTexture(3, None)
        with pytest.raises(P.PtException) as e:
            renderer.Render(0.0)
        assert e.value.status == 5  # PT_ERR_NOT_COMMITTED: a setter marks the scene uncommitted
        renderer.Commit(0)
        for nee in (False, True):
            renderer.Params = params_of(P, nee, spp=4, max_depth=8, streams=2)
            renderer.Render(0.0)
            assert np.array_equal(renderer.ReadFramebuffer().view(np.uint32), frames[nee][1].view(np.uint32)), (remove, nee)


def test_update_geometry_keeps_the_texturing(P, pto, renderer):
    """pt_scene_update_triangles keeps the UVs: the moved scene's frame is the checker's, and a fresh commit of the moved vertices with the
    same UVs gives the same frame."""
    sd = two_textures(P, "cornell")
    v2 = sd.verts.copy()
    v2[:, 1::3] *= 0.9  # squash the box
    moved = dataclasses.replace(sd, verts=v2)
    for width in (0, 68):
        renderer.SetScene(sd, width)
        renderer.UpdateGeometry(verts=v2)
        for nee in (False, True):
            params = params_of(P, nee, spp=4, max_depth=8, streams=2)
            check(P, pto, renderer, moved, params, None, ("updated", width, nee))
        updated = renderer.ReadFramebuffer()
        renderer.SetScene(moved, width)
        renderer.Render(0.0)
        assert np.array_equal(renderer.ReadFramebuffer().view(np.uint32), updated.view(np.uint32)), width
        assert renderer.TextureInfo(0).materials == 1 and renderer.TextureInfo(3).materials == 2


def test_progressive_and_multi_rank(P, pto, renderer, sun):
    """Four accumulate calls of 4 spp, and two virtual ranks on one context, give the one-shot frame."""
    N = P.native
    sd = with_env(two_textures(P, "cornell"), sun)
    renderer.SetScene(sd, 0)
    for nee in (False, True):
        whole, _ = check(P, pto, renderer, sd, params_of(P, nee, spp=16, max_depth=8, streams=4), sun, ("whole", nee))
        want = renderer.ReadFramebuffer()
        rays = 0
        for k in range(4):
            p = params_of(P, nee, spp=4, max_depth=8, streams=4, sample_offset=4 * k)
            if k:
                p.flags |= N.PT_FLAG_ACCUMULATE
            renderer.Params = p
            rays += renderer.Render(0.0).rays
        assert np.array_equal(renderer.ReadFramebuffer(), want) and rays == whole.rays, nee
        with P.Comm([renderer] * 2, root=1) as comm:
            stats = comm.Render(params_of(P, nee, spp=16, max_depth=8, streams=4))
            assert sum(s.rays for s in stats) == whole.rays and sum(s.paths for s in stats) == whole.paths
            assert np.array_equal(renderer.ReadFramebuffer(), want), nee


def test_guides_carry_the_textured_albedo(P, pto, renderer):
    """ReadGuides' g1.rgb = albedo * lookup at TraceRays' (u, v) of the guide rays, bit for bit, for triangle hits of bound materials;
    spheres and everything else of the guides equal the untextured scene's."""
    plain = P.make_scene(P.native.PT_SCENE_CORNELL_GLASS, 0, 3, W, H)
    renderer.SetScene(plain, 0)
    renderer.Params = params_of(P, False, spp=2, max_depth=4, streams=1)
    renderer.Render(0.0)
    renderer.Denoise(iterations=1)
    g_plain = renderer.ReadGuides()
    tex = {0: tc.distinct(3, 5), 3: tc.distinct(4, 4, 40)}
    sd = tc.cornell(P, W, H, tex[0], (tex[3], tc.NEAREST), glass=True)
    renderer.SetScene(sd, 0)
    renderer.Render(0.0)
    st = renderer.Denoise(iterations=1)
    assert st.rays == W * H
    g = renderer.ReadGuides()
    assert np.array_equal(g[..., :4].view(np.uint32), g_plain[..., :4].view(np.uint32))  # g0
    assert np.array_equal(g[..., 7].view(np.uint32), g_plain[..., 7].view(np.uint32))    # the ids
    hits, _ = renderer.TraceRays(jitter_free_rays(pto, sd.cam))
    ids = np.ascontiguousarray(hits[:, 1]).view(np.uint32)
    assert np.array_equal(ids, np.ascontiguousarray(g[..., 7]).view(np.uint32).reshape(-1))
    want = g_plain[..., 4:7].reshape(-1, 3).copy()
    n_tex = 0
    for i in np.nonzero(ids < len(sd.tri_mat))[0]:
        m = sd.tri_mat[ids[i]]
        t = sd.material_textures[m]
        if t == tc.NO_TEXTURE:
            continue
        s_, t_ = tc.coordinate(sd.uvs[ids[i]], hits[i, 2], hits[i, 3])
        want[i] = sd.mats[m]["albedo"].astype(np.float32) * tc.lookup(tex[int(t)], s_, t_, tc.NEAREST if t == 3 else 0)
        n_tex += 1
    assert n_tex > W * H // 3
    assert np.array_equal(g[..., 4:7].reshape(-1, 3).view(np.uint32), want.view(np.uint32))
    assert not np.array_equal(g[..., 4:7], g_plain[..., 4:7]) and np.isfinite(renderer.ReadDenoised()).all()


def test_refusals_and_the_context_still_renders(P, pto, renderer, sun):
    """Every request docs/SPEC.md §13 refuses, with its status and a message that says why; the next ordinary frame is right."""
    N = P.native
    sd = two_textures(P, "cornell")
    renderer.SetScene(sd, 0)
    for nee in (False, True):
        for name in ("EXTEND_PACKED", "EXTEND_POOL", "SPLIT_KERNELS", "BUCKET_SPECULAR", "COUNT_VISITS"):
            p = params_of(P, nee, spp=2, max_depth=8)
            p.flags |= FLAGS[name]
            renderer.Params = p
            with pytest.raises(P.PtException, match="textured") as e:
                renderer.Render(0.0)
            assert e.value.status == PT_ERR_UNSUPPORTED, name
    tuning = renderer.GetTuning().extend_kernel
    try:
        for k in (2, 3):
            renderer.SetTuning(extend_kernel=k)
            renderer.Params = params_of(P, False, spp=2, max_depth=8)
            with pytest.raises(P.PtException, match="textured") as e:
                renderer.Render(0.0)
            assert e.value.status == PT_ERR_UNSUPPORTED, k
    finally:
        renderer.SetTuning(extend_kernel=tuning)
    renderer.SetLens(0.05, 3.0)
    renderer.Params = params_of(P, False, spp=2, max_depth=8)
    with pytest.raises(P.PtException, match="lens") as e:
        renderer.Render(0.0)
    assert e.value.status == PT_ERR_UNSUPPORTED
    renderer.SetLens(0.0, 3.0)  # radius 0 is no lens
    check(P, pto, renderer, sd, params_of(P, True, spp=4, max_depth=8, streams=2), None, "radius 0")
    renderer.ClearLens()
    pts = np.array([[0.0, -0.99, 0.0]], np.float32)
    with pytest.raises(P.PtException, match="textured") as e:
        renderer.GatherPaths(pts, np.array([[0.0, 1.0, 0.0]], np.float32), samples=4)
    assert e.value.status == PT_ERR_UNSUPPORTED
    renderer.Gather(pts, np.array([[0.0, 1.0, 0.0]], np.float32), samples=4)  # pt_gather does not look at textures
    # a sphere light: PT_FLAG_NEXT_EVENT_SPHERES is refused, PT_FLAG_NEXT_EVENT alone is the checker's frame
    mats = sd.mats.copy()
    mats[4]["emission"] = (4.0, 4.0, 4.0)
    lit = dataclasses.replace(sd, mats=mats, sph_mat=np.array([0, 4, 5, 0], np.uint32))
    renderer.SetScene(lit, 0)
    p = params_of(P, True, spp=2, max_depth=8)
    p.flags |= N.PT_FLAG_NEXT_EVENT_SPHERES
    renderer.Params = p
    with pytest.raises(P.PtException, match="sphere light") as e:
        renderer.Render(0.0)
    assert e.value.status == PT_ERR_UNSUPPORTED
    check(P, pto, renderer, lit, params_of(P, True, spp=4, max_depth=8, streams=2), None, "sphere light, triangle NEE")
    renderer.SetScene(sd, 0)  # without a sphere light the flag is PT_FLAG_NEXT_EVENT's frame
    p = params_of(P, True, spp=4, max_depth=8, streams=2)
    ref, cst = reference(pto, sd, p, None, True)
    p.flags |= N.PT_FLAG_NEXT_EVENT_SPHERES
    renderer.Params = p
    same_frame(P, renderer, ref, cst, "no sphere light")
    for nee in (False, True):
        p = params_of(P, nee, spp=4, max_depth=8, streams=2)
        p.flags |= N.PT_FLAG_EXTEND_SIMPLE | N.PT_FLAG_PROFILE_KERNELS  # the kernel these frames run on, forced, and timed: accepted
        check(P, pto, renderer, sd, p, None, ("after refusals", nee))
