"""-m gpu: sphere lights in next-event estimation (PT_FLAG_NEXT_EVENT | PT_FLAG_NEXT_EVENT_SPHERES, docs/SPEC.md §7.1) on the device against
the scalar checker of tests/sphere_light_ref/.

Every frame is compared bit for bit, with `rays` equal to the checker's extension plus shadow rays. Frames are 20 x 12 at 4 spp: partial
8 x 8 blocks, and lanes of one wave that choose triangles, spheres and the map side by side. Every test commits its own scene on the
session's renderer."""
import dataclasses

import numpy as np
import pytest

import nee_checker as nc
import sphere_light_checker as sc
from pipelines import refused
from trace_support import LAYOUTS

pytestmark = pytest.mark.gpu
W, H, SPP = 20, 12, 4
LENS = (0.05, 3.0)
_refs = {}


def flagged(P, **kw):
    return P.make_params(W, H, next_event=True, sphere_lights=True, **{"spp": SPP, "max_depth": 8, "streams": 2, **kw})


def reference(P, pto, name, sd, env, lens, params, flags=sc.FLAGGED):
    """The checker's frame, computed once per (scene name, what lights it, the frame's parameters) and left unchanged."""
    key = (name, env is not None, lens, params.spp, params.streams, params.max_depth, params.sample_offset, flags)
    if key not in _refs:
        _refs[key] = sc.render(pto, pto.Scene(sd), params, env=env, lens=lens, flags=flags)[:2]
    return _refs[key]


def check(P, pto, r, name, sd, env, lens, params, ctx, flags=sc.FLAGGED):
    """The renderer's frame of its current scene = the checker's, bit for bit; rays = extension + shadow rays."""
    r.Params = params
    st = r.Render(0.0)
    img = r.ReadFramebuffer()
    ref, cst = reference(P, pto, name, sd, env, lens, params, flags)
    assert np.isfinite(img).all(), ctx
    bad = np.argwhere((img != ref).any(axis=2))
    assert len(bad) == 0, (ctx, len(bad), bad[:4].tolist(), img[tuple(bad[0])].tolist() if len(bad) else None,
                           ref[tuple(bad[0])].tolist() if len(bad) else None)
    assert st.rays == cst.ext_rays + cst.shadow_rays, (ctx, st.rays, cst.ext_rays, cst.shadow_rays)
    assert st.paths == cst.paths, (ctx, st.paths, cst.paths)
    return st, cst


CASES = {"lamp": ("lamp", False, None), "lamp+quad": ("lamp+quad", False, None), "lamp+quad+map": ("lamp+quad", True, None),
         "lamp+quad+map+lens": ("lamp+quad", True, LENS), "lamp+lens": ("lamp", False, LENS), "glass-lamp": ("glass-lamp", False, None)}


def commit(P, r, name, width=0):
    """Commits case `name` on the renderer: (scene data, map or None, lens or None)."""
    scene, with_map, lens = CASES[name]
    sd = sc.scene(P, scene, W, H)
    env = sc.lit_map(P) if with_map else None
    r.SetScene(sd if env is None else dataclasses.replace(sd, environment=env), width)
    if lens:
        r.SetLens(*lens)
    return sd, env, lens


# ---------------------------------------------------------------------------------------------------------------------- 9. bit identity
@pytest.mark.parametrize("name", list(CASES))
def test_layouts_and_builders(P, pto, renderer, name):
    """All five layouts x both builders, lit by a lamp only, a lamp and the quad, those under a lit map, and the same through a lens: the
    checker's frame and ray count."""
    N = P.native
    for width in LAYOUTS:
        for build in (0, N.PT_BVH_BUILD_LBVH):
            sd, env, lens = commit(P, renderer, name, width | build)
            st, cst = check(P, pto, renderer, name, sd, env, lens, flagged(P), (name, width, build))
            assert cst.n_sphere_lights >= 1 and cst.shadow_rays > 0 and (cst.lit == 1) == (env is not None)


@pytest.mark.parametrize("streams", [1, 8])
@pytest.mark.parametrize("depth", [1, 2, 8])
def test_streams_and_depths(P, pto, renderer, streams, depth):
    for name in ("lamp+quad", "lamp+quad+map"):
        sd, env, lens = commit(P, renderer, name)
        st, cst = check(P, pto, renderer, name, sd, env, lens, flagged(P, spp=8, max_depth=depth, streams=streams), (name, streams, depth))
        assert (cst.shadow_rays == 0) == (depth == 1)  # no vertex below max_depth: the plain frame


def test_progressive_and_ranks(P, pto, renderer):
    """A 3 + 5 split with PT_FLAG_ACCUMULATE is the 8-sample frame; three virtual ranks assemble the single-rank frame."""
    N = P.native
    sd, env, lens = commit(P, renderer, "lamp+quad+map")
    whole, _ = check(P, pto, renderer, "lamp+quad+map", sd, env, lens, flagged(P, spp=8, streams=4), "whole")
    want = renderer.ReadFramebuffer()
    rays = 0
    for off, n in ((0, 3), (3, 5)):
        p = flagged(P, spp=n, streams=4, sample_offset=off)
        if off:
            p.flags |= N.PT_FLAG_ACCUMULATE
        renderer.Params = p
        rays += renderer.Render(0.0).rays
    assert np.array_equal(renderer.ReadFramebuffer(), want) and rays == whole.rays
    with P.Comm([renderer] * 3, root=2) as comm:
        stats = comm.Render(flagged(P, spp=8, streams=4))
        assert sum(s.rays for s in stats) == whole.rays and sum(s.paths for s in stats) == whole.paths
        assert np.array_equal(renderer.ReadFramebuffer(), want)


# --------------------------------------------------------------------------------------------------------------------- 10. moving a lamp
def test_updates_move_the_lamp(P, pto, renderer):
    """After pt_scene_update_spheres moves and resizes the lamp, and after pt_scene_update_triangles moves the quad, the frame equals
    the checker's on the updated scene and the frame of a fresh commit."""
    N = P.native
    sd = sc.scene(P, "lamp+quad", W, H)
    sph = sd.spheres.copy()
    sph[-1] = (0.4, 0.2, -0.3, 0.25)  # the lamp is the last sphere: elsewhere, and bigger
    light = np.nonzero(sd.mats["emission"].sum(axis=1)[sd.tri_mat] > 0)[0]
    v2 = sd.verts.copy()
    q = v2[light].reshape(-1, 3, 3)
    q[:, :, 0] = q[:, :, 0] * 1.5 + 0.2
    q[:, :, 1] -= 0.3
    v2[light] = q.reshape(-1, 9)
    steps = (("lamp moved", dataclasses.replace(sd, spheres=sph), dict(spheres=sph)),
             ("lamp and quad moved", dataclasses.replace(sd, spheres=sph, verts=v2), dict(verts=v2)))
    for width in (2, 68 | N.PT_BVH_BUILD_LBVH, 73):
        fresh = {}
        for name, moved, _ in steps:
            renderer.SetScene(moved, width)
            check(P, pto, renderer, name, moved, None, None, flagged(P), ("fresh", name, width))
            fresh[name] = renderer.ReadFramebuffer()
        renderer.SetScene(sd, width)
        check(P, pto, renderer, "lamp+quad", sd, None, None, flagged(P), ("before", width))
        for name, moved, update in steps:  # the second update is applied on top of the first
            renderer.UpdateGeometry(**update)
            check(P, pto, renderer, name, moved, None, None, flagged(P), (name, width))
            assert np.array_equal(renderer.ReadFramebuffer(), fresh[name]), (name, width)
        assert not np.array_equal(fresh["lamp moved"], fresh["lamp and quad moved"])


# ----------------------------------------------------------------------------------------------------- 11. unflagged frames unchanged
def test_unflagged_frames_are_unchanged(P, pto, renderer):
    """On the same scenes an unflagged PT_FLAG_NEXT_EVENT frame still equals nee_checker and a plain frame the oracle; a flagged frame on
    a scene without sphere lights is the unflagged frame bit for bit, with the same rays."""
    for name in ("lamp", "lamp+quad", "glass-lamp"):
        sd, _, _ = commit(P, renderer, name)
        p = P.make_params(W, H, spp=SPP, max_depth=8, streams=2, next_event=True)
        renderer.Params = p
        st = renderer.Render(0.0)
        ref, cst, _ = nc.render(pto, pto.Scene(sd), p)
        assert np.array_equal(renderer.ReadFramebuffer(), ref) and st.rays == cst.ext_rays + cst.shadow_rays, name
        p = P.make_params(W, H, spp=SPP, max_depth=8, streams=2)
        renderer.Params = p
        st = renderer.Render(0.0)
        ref, ost = pto.render(pto.Scene(sd), p)
        assert np.array_equal(renderer.ReadFramebuffer(), ref) and st.rays == ost.rays, name
    for sd in (P.make_scene(P.native.PT_SCENE_CORNELL_GLASS, 0, 3, W, H), sc.without_sphere_emission(nc.many_lights_scene(P, W, H))):
        renderer.SetScene(sd, 0)
        renderer.Params = P.make_params(W, H, spp=SPP, max_depth=8, streams=2, next_event=True)
        a = renderer.Render(0.0)
        img = renderer.ReadFramebuffer()
        renderer.Params = flagged(P)
        b = renderer.Render(0.0)
        assert np.array_equal(renderer.ReadFramebuffer(), img) and a.rays == b.rays and a.paths == b.paths


# ------------------------------------------------------------------------------------------------------------------------ 12. refusals
def test_refusals(P, pto, renderer):
    """512 without 256, mixed settings under PT_FLAG_ACCUMULATE and every pipeline NEE refuses, also with the flag: refused before the
    frame replaces anything — the previous frame is intact — and the context renders the next frame correctly."""
    N = P.native
    sd, env, lens = commit(P, renderer, "lamp+quad")
    check(P, pto, renderer, "lamp+quad", sd, env, lens, flagged(P), "first")
    kept = renderer.ReadFramebuffer()

    def refused_with(params, status, match=None):
        renderer.Params = params
        with pytest.raises(P.PtException, match=match) as e:
            renderer.Render(0.0)
        assert e.value.status == status, (e.value.status, status)
        assert np.array_equal(renderer.ReadFramebuffer(), kept)

    refused_with(P.make_params(W, H, spp=SPP, streams=2, flags=N.PT_FLAG_NEXT_EVENT_SPHERES), N.PT_ERR_INVALID_ARGUMENT, "NEXT_EVENT_SPHERES")
    p = P.make_params(W, H, spp=SPP, streams=2, next_event=True, sample_offset=SPP, flags=N.PT_FLAG_ACCUMULATE)
    refused_with(p, N.PT_ERR_INVALID_ARGUMENT, "NEXT_EVENT_SPHERES")  # flagged sums are not continued without the flag ...
    for flags in [r.flags for r in refused("nee")]:
        p = flagged(P)
        p.flags |= flags
        refused_with(p, N.PT_ERR_UNSUPPORTED)
    tuning = renderer.GetTuning().extend_kernel
    try:
        for k in [r.tuned_kernel for r in refused("nee", tuned=True)]:
            renderer.SetTuning(extend_kernel=k)
            refused_with(flagged(P), N.PT_ERR_UNSUPPORTED)
    finally:
        renderer.SetTuning(extend_kernel=tuning)
    renderer.Params = P.make_params(W, H, spp=SPP, streams=2, next_event=True)
    renderer.Render(0.0)
    kept = renderer.ReadFramebuffer()
    p = flagged(P, sample_offset=SPP)
    p.flags |= N.PT_FLAG_ACCUMULATE
    refused_with(p, N.PT_ERR_INVALID_ARGUMENT, "NEXT_EVENT_SPHERES")  # ... nor unflagged sums with it
    p = flagged(P)
    p.flags |= N.PT_FLAG_EXTEND_SIMPLE | N.PT_FLAG_PROFILE_KERNELS  # the kernel it runs on, forced, and timed: accepted
    check(P, pto, renderer, "lamp+quad", sd, env, lens, p, "after refusals")
