"""-m gpu: pt_denoise (docs/SPEC.md §8) on the device against the scalar checker of tests/denoise_ref/.

The guides and the denoised image are compared bit for bit (the checker filters the device's own framebuffer), with rays = W*H, over
every BVH layout and both builders, scenes with triangles, spheres and sky, frame sizes from 1x1 to 1920x1080, every pass count, both
flags, frames assembled from virtual ranks and updated geometry. Also: what a denoise leaves alone, when its results expire, every
refusal, and the quality it buys on the Cornell boxes."""
import dataclasses

import numpy as np
import pytest

import denoise_checker as dc
from frame_checks import check_denoise as check
from trace_support import LAYOUTS

pytestmark = pytest.mark.gpu


def sky_scene(P, w, h):
    """C4 (triangles, glass / metal / Lambert spheres) seen from further back, so that the sky shows around the open box."""
    sd = P.make_scene(P.native.PT_SCENE_CORNELL_GLASS, 0, 3, w, h)
    cam = type(sd.cam)()
    cam.origin[:] = (0.3, 0.2, 4.5)
    f = np.array([-0.05, -0.03, -1.0]); f /= np.linalg.norm(f)
    r = np.cross(f, [0.0, 1.0, 0.0]); r /= np.linalg.norm(r)
    u = np.cross(r, f)
    cam.forward[:], cam.right[:], cam.up[:] = f.tolist(), (r * 0.3).tolist(), (u * 0.3).tolist()
    cam.scale, cam.cx, cam.cy, cam.jitter = 2.0 / h, w / h, 1.0, 1
    return dataclasses.replace(sd, cam=cam, sky=np.array([0.3, 0.4, 0.6], np.float32))


@pytest.mark.parametrize("name", ["cornell", "sky"])
def test_layouts_and_builders(P, pto, renderer, name):
    N = P.native
    w, h = 67, 45
    sd = P.make_scene(N.PT_SCENE_CORNELL, 0, 3, w, h) if name == "cornell" else sky_scene(P, w, h)
    for width in LAYOUTS:
        for build in (0, N.PT_BVH_BUILD_LBVH):
            renderer.SetScene(sd, width | build)
            renderer.Params = P.make_params(w, h, spp=2, max_depth=6, streams=2)
            renderer.Render(0.0)
            _, g, _ = check(P, pto, renderer, sd, (name, width, build))
            ids = g[..., 7].view(np.uint32)
            assert (ids < len(sd.tri_mat)).any() and (ids == dc.MISS).any()
            assert ((ids >= len(sd.tri_mat)) & (ids != dc.MISS)).any()  # spheres


def test_tessellated_scene(P, pto, renderer):
    """Thousands of triangles on the default layout, both builders: the id -> blob index table of a real tree."""
    N = P.native
    sd = P.make_scene(N.PT_SCENE_CORNELL_TESS, 3000, 3, 96, 64)
    for build in (0, N.PT_BVH_BUILD_LBVH):
        renderer.SetScene(sd, N.PT_BVH_WIDTH_4Q | build)
        renderer.Params = P.make_params(96, 64, spp=2, max_depth=4)
        renderer.Render(0.0)
        check(P, pto, renderer, sd, build)


@pytest.mark.parametrize("w,h", [(1, 1), (7, 3), (67, 45), (320, 200), (1920, 1080)])
def test_sizes(P, pto, renderer, w, h):
    sd = sky_scene(P, w, h)
    renderer.SetScene(sd, 0)
    renderer.Params = P.make_params(w, h, spp=1, max_depth=4)
    renderer.Render(0.0)
    st, _, _ = check(P, pto, renderer, sd, (w, h))
    assert st.gpu_ms > 0 and st.extend_ms > 0 and st.other_ms > 0 and st.iterations == dc.defaults()[0]


def test_iterations_sigmas_and_flags(P, pto, renderer):
    w, h = 80, 60
    sd = sky_scene(P, w, h)
    renderer.SetScene(sd, 0)
    renderer.Params = P.make_params(w, h, spp=2, max_depth=6)
    renderer.Render(0.0)
    for it in range(1, 9):
        st, _, _ = check(P, pto, renderer, sd, it, iterations=it)
        assert st.iterations == it
    check(P, pto, renderer, sd, "sigmas", iterations=4, sigma_color=0.5, sigma_normal=0.3, sigma_depth=0.2, sigma_albedo=0.1)
    check(P, pto, renderer, sd, "no edge stops", iterations=5, edge_stops=False)
    st, _, _ = check(P, pto, renderer, sd, "guides only", guides_only=True)
    assert st.iterations == 0


def test_virtual_ranks(P, pto, renderer):
    """A frame assembled from three virtual ranks through pt_comm is denoised like the single-rank frame."""
    w, h = 150, 100
    sd = sky_scene(P, w, h)
    renderer.SetScene(sd, 0)
    params = P.make_params(w, h, spp=2, max_depth=6, streams=2)
    renderer.Params = params
    renderer.Render(0.0)
    one = renderer.Denoise()
    want = renderer.ReadDenoised()
    with P.Comm([renderer] * 3, root=1) as comm:
        comm.Render(P.make_params(w, h, spp=2, max_depth=6, streams=2))
        check(P, pto, renderer, sd, "comm")
        assert np.array_equal(renderer.ReadDenoised(), want) and one.rays == w * h


def test_after_update(P, pto, renderer):
    """After pt_scene_update_triangles moves geometry the guides follow it (the id -> blob table is kept, the records moved)."""
    N = P.native
    w, h = 64, 48
    sd = P.make_scene(N.PT_SCENE_CORNELL_GLASS, 0, 3, w, h)
    v2 = sd.verts.copy().reshape(-1, 3, 3)
    v2[:, :, 0] += 0.15 * np.sin(np.arange(len(v2)))[:, None]
    v2[:, :, 2] -= 0.1
    moved = dataclasses.replace(sd, verts=v2.reshape(-1, 9))
    for width in (2, 68, 73):
        renderer.SetScene(sd, width)
        renderer.Params = P.make_params(w, h, spp=2, max_depth=4)
        renderer.Render(0.0)
        check(P, pto, renderer, sd, ("before", width))  # builds the table
        renderer.UpdateGeometry(verts=moved.verts)
        renderer.Render(0.0)
        check(P, pto, renderer, moved, ("after", width))


def test_state(P, pto, renderer):
    """A denoise leaves the framebuffer and the accumulated sums alone; the next pt_render expires its results."""
    N = P.native
    w, h = 64, 48
    sd = P.make_scene(N.PT_SCENE_CORNELL, 0, 3, w, h)
    renderer.SetScene(sd, 0)
    acc = P.make_params(w, h, spp=2, max_depth=6, streams=2)
    renderer.Params = acc
    renderer.Render(0.0)
    before = renderer.ReadFramebuffer()
    renderer.Denoise()
    assert np.array_equal(renderer.ReadFramebuffer(), before)
    for p in (P.make_params(w, h, spp=2, max_depth=6, streams=2, flags=N.PT_FLAG_ACCUMULATE, sample_offset=2),
              P.make_params(w, h, spp=3, max_depth=6, streams=2, flags=N.PT_FLAG_ACCUMULATE, sample_offset=4)):
        renderer.Params = p
        renderer.Render(0.0)
        renderer.Denoise(iterations=2)
    with_denoise = renderer.ReadFramebuffer()
    for p in (acc, P.make_params(w, h, spp=2, max_depth=6, streams=2, flags=N.PT_FLAG_ACCUMULATE, sample_offset=2),
              P.make_params(w, h, spp=3, max_depth=6, streams=2, flags=N.PT_FLAG_ACCUMULATE, sample_offset=4)):
        renderer.Params = p
        renderer.Render(0.0)
    assert np.array_equal(renderer.ReadFramebuffer(), with_denoise)
    renderer.Denoise()
    renderer.ReadDenoised(); renderer.ReadGuides()
    renderer.Params = acc
    renderer.Render(0.0)
    for read in (renderer.ReadDenoised, renderer.ReadGuides):
        with pytest.raises(P.PtException) as e:
            read()
        assert e.value.status == N.PT_ERR_NOT_COMMITTED


def test_refusals(P, pto, renderer):
    """Each refusal returns its status, changes nothing, and the context goes on working."""
    import ctypes as C
    N, lib = P.native, P.native.lib
    w, h = 32, 24
    sd = P.make_scene(N.PT_SCENE_CORNELL, 0, 3, w, h)
    renderer.SetScene(sd, 0)
    renderer.Params = P.make_params(w, h, spp=1, max_depth=4)
    renderer.Render(0.0)
    renderer.Denoise()
    kept = renderer.ReadDenoised()

    def status(**kw):
        with pytest.raises(P.PtException) as e:
            renderer.Denoise(**kw)
        return e.value.status

    assert status(iterations=9) == N.PT_ERR_INVALID_ARGUMENT
    assert status(sigma_color=-1.0) == N.PT_ERR_INVALID_ARGUMENT
    assert status(sigma_depth=float("nan")) == N.PT_ERR_INVALID_ARGUMENT
    dp = N.pt_denoise_params(0, 0, 0, 0, 0, 8)
    assert lib.pt_denoise(renderer._ctx, renderer._scene, C.byref(dp), None) == N.PT_ERR_INVALID_ARGUMENT
    dp.flags = 0
    assert lib.pt_denoise(renderer._ctx, None, C.byref(dp), None) == N.PT_ERR_INVALID_ARGUMENT
    assert lib.pt_denoise(renderer._ctx, renderer._scene, None, None) == N.PT_ERR_INVALID_ARGUMENT
    assert np.array_equal(renderer.ReadDenoised(), kept)  # refused calls changed nothing
    # a detached scene, a scene of another context, an uncommitted scene
    det = C.c_void_p()
    assert lib.pt_scene_create(None, C.byref(det)) == 0
    other = P.Renderer(P.Window(w, h))
    other.Init()
    unc = C.c_void_p()
    assert lib.pt_scene_create(renderer._ctx, C.byref(unc)) == 0
    try:
        assert lib.pt_denoise(renderer._ctx, det, C.byref(dp), None) == N.PT_ERR_UNSUPPORTED
        other.SetScene(sd, 0)
        assert lib.pt_denoise(renderer._ctx, other._scene, C.byref(dp), None) == N.PT_ERR_UNSUPPORTED
        assert lib.pt_denoise(renderer._ctx, unc, C.byref(dp), None) == N.PT_ERR_NOT_COMMITTED
        # no assembled frame on `other` yet
        assert lib.pt_denoise(other._ctx, other._scene, C.byref(dp), None) == N.PT_ERR_NOT_COMMITTED
    finally:
        lib.pt_scene_destroy(det)
        lib.pt_scene_destroy(unc)
        other.Dispose()
    assert np.array_equal(renderer.ReadDenoised(), kept)
    # a PT_REFERENCE_SPHERE frame
    renderer.Params = P.make_params(w, h, mode=N.PT_REFERENCE_SPHERE)
    renderer.Render(0.0)
    assert status() == N.PT_ERR_UNSUPPORTED
    # a frame of several ranks without assembly leaves no framebuffer
    renderer.Params = P.make_params(w, h, spp=1, max_depth=4, rank=0, nranks=2)
    renderer.Render(0.0)
    assert status() == N.PT_ERR_NOT_COMMITTED
    # and the context still works
    renderer.Params = P.make_params(w, h, spp=1, max_depth=4)
    renderer.Render(0.0)
    check(P, pto, renderer, sd, "after refusals")


def display_rmse(a, ref):
    """RMSE of the displayed image: radiance clamped to [0, 1], what the 8-bit framebuffer shows (SPEC §1 unorm8)."""
    return float(np.sqrt(np.mean((np.clip(a[..., :3].astype(np.float64), 0, 1) - np.clip(ref[..., :3].astype(np.float64), 0, 1)) ** 2)))


def test_quality(P, renderer):
    """4 spp frames (960 x 540) of C1 with NEE and of C4 against converged device frames (16384 spp): the denoised frame's displayed error is at
    least 2x lower than the noisy frame's; and at geometric edges (a guide id differs from a 4-neighbour) the guided filter beats
    the plain blur, which is what the guides are for."""
    N = P.native
    w, h = 960, 540
    for kind, flags in ((N.PT_SCENE_CORNELL, N.PT_FLAG_NEXT_EVENT), (N.PT_SCENE_CORNELL_GLASS, 0)):
        sd = P.make_scene(kind, 0, 3, w, h)
        renderer.SetScene(sd, 0)
        renderer.Params = P.make_params(w, h, spp=16384, max_depth=8, streams=8, seed=99, flags=flags)
        renderer.Render(0.0)
        ref = renderer.ReadFramebuffer()
        renderer.Params = P.make_params(w, h, spp=4, max_depth=8, streams=4, seed=7, flags=flags)
        renderer.Render(0.0)
        noisy = renderer.ReadFramebuffer()
        renderer.Denoise()
        den = renderer.ReadDenoised()
        ids = renderer.ReadGuides()[..., 7].view(np.uint32)
        renderer.Denoise(edge_stops=False)
        blur = renderer.ReadDenoised()
        e_noisy, e_den = display_rmse(noisy, ref), display_rmse(den, ref)
        assert e_den * 2 <= e_noisy, (kind, e_noisy, e_den)
        edge = np.zeros(ids.shape, bool)
        edge[:, 1:] |= ids[:, 1:] != ids[:, :-1]; edge[:, :-1] |= ids[:, 1:] != ids[:, :-1]
        edge[1:] |= ids[1:] != ids[:-1]; edge[:-1] |= ids[1:] != ids[:-1]
        err = lambda a: float(np.sqrt(np.mean((a[edge][:, :3].astype(np.float64) - ref[edge][:, :3]) ** 2)))  # noqa: E731
        assert err(den) < err(blur), (kind, err(den), err(blur))
