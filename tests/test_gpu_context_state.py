"""-m gpu: what a context still holds after each public call, pinned at the transitions that csrc/context.h makes in one place each.

The framebuffer and the denoised results after a refused pt_render and after pt_assemble_tiles, the partial sums after a refused
PT_FLAG_ACCUMULATE frame, the frame-start template across the two queue-size read-back modes, and the tile block after a frame of
another kind. Every test runs the 12-triangle Cornell box at 32 x 24, 1-2 spp, depth 4, on a context of its own, so that no state of
another test is in play. (Denoised results dying at the next render, pt_denoise's refusal of a reference frame and the multi-rank
frame without assembly are covered by test_gpu_denoise.py.)"""
import contextlib
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 32, 24


@pytest.fixture(scope="module")
def box(P):
    return P.make_scene(P.native.PT_SCENE_CORNELL, 0, 3, W, H)


@contextlib.contextmanager
def context(P, sd):
    r = P.Renderer(P.Window(W, H))
    r.Init()
    try:
        r.SetScene(sd, 0)
        yield r
    finally:
        r.Dispose()


def frame(P, **kw):
    kw = {"spp": 2, "max_depth": 4, "streams": 2, **kw}
    return P.make_params(W, H, **kw)


def render(P, r, **kw):
    r.Params = frame(P, **kw)
    st = r.Render(0.0)
    return r.ReadFramebuffer(), st


def refused(P, call, status, *words):
    with pytest.raises(P.PtException) as e:
        call()
    assert e.value.status == status, str(e.value)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def plain(P, box):
    """The plain frame of a context that has done nothing else: (pixels, rays)."""
    with context(P, box) as r:
        img, st = render(P, r)
        return img, int(st.rays)


def nothing_readable(P, r):
    N = P.native
    refused(P, r.ReadFramebuffer, N.PT_ERR_NOT_COMMITTED)
    refused(P, r.ReadDenoised, N.PT_ERR_NOT_COMMITTED)
    refused(P, r.ReadGuides, N.PT_ERR_NOT_COMMITTED)


@pytest.mark.parametrize("how", ["spp_zero", "uncommitted_scene"])
def test_refused_render_leaves_nothing(P, box, plain, how):
    """A pt_render refused after it has begun to replace the frame: no framebuffer, no denoised image, no guides, no sums to continue;
    and the next plain frame is the one a fresh context renders."""
    N = P.native
    with context(P, box) as r:
        render(P, r)
        r.Denoise()
        assert r.ReadDenoised().shape == (H, W, 4) and r.ReadGuides().shape == (H, W, 8)
        if how == "spp_zero":
            r.Params = frame(P, spp=0)
            refused(P, lambda: r.Render(0.0), N.PT_ERR_INVALID_ARGUMENT, "spp must be in")
        else:
            s = C.c_void_p()
            assert N.lib.pt_scene_create(r._ctx, C.byref(s)) == N.PT_OK
            try:
                p, st = frame(P), N.pt_stats()
                assert N.lib.pt_render(r._ctx, s, C.byref(p), C.byref(st)) == N.PT_ERR_NOT_COMMITTED
                assert b"scene not committed" in N.lib.pt_last_error(r._ctx)
            finally:
                N.lib.pt_scene_destroy(s)
        r.Params = frame(P)
        nothing_readable(P, r)
        r.Params = frame(P, sample_offset=2, flags=N.PT_FLAG_ACCUMULATE)
        refused(P, lambda: r.Render(0.0), N.PT_ERR_INVALID_ARGUMENT, "needs a previous frame")
        img, st = render(P, r)
        assert same(img, plain[0]) and st.rays == plain[1]


def test_render_without_params(P, box, plain):
    """pt_render(params = NULL) is refused before render_frame invalidates anything, but pt_render's own failure path still runs: the
    framebuffer stops being readable and the sums stop being continuable, while the denoised image and the guides — which only the
    start of a frame drops — still read back unchanged. Stale-looking, and pinned as it is."""
    N = P.native
    with context(P, box) as r:
        img, _ = render(P, r)
        assert same(img, plain[0])
        r.Denoise()
        dn, g = r.ReadDenoised(), r.ReadGuides()
        st = N.pt_stats()
        assert N.lib.pt_render(r._ctx, r._scene, None, C.byref(st)) == N.PT_ERR_INVALID_ARGUMENT
        assert b"pt_render: NULL argument" in N.lib.pt_last_error(r._ctx)
        refused(P, r.ReadFramebuffer, N.PT_ERR_NOT_COMMITTED)
        assert same(r.ReadDenoised(), dn) and same(r.ReadGuides(), g)
        r.Params = frame(P, sample_offset=2, flags=N.PT_FLAG_ACCUMULATE)
        refused(P, lambda: r.Render(0.0), N.PT_ERR_INVALID_ARGUMENT, "needs a previous frame")
        img, st = render(P, r)
        assert same(img, plain[0]) and st.rays == plain[1]


def test_assemble_drops_denoised_results(P, box, plain):
    import torch
    with context(P, box) as r:
        img, _ = render(P, r)
        r.Denoise()
        r.ReadDenoised(), r.ReadGuides()
        tiles = torch.as_tensor(r.TilesDevice(), device="cuda").clone()
        torch.cuda.synchronize()
        r.AssembleTiles(tiles.data_ptr(), tiles.numel())
        N = P.native
        refused(P, r.ReadDenoised, N.PT_ERR_NOT_COMMITTED)
        refused(P, r.ReadGuides, N.PT_ERR_NOT_COMMITTED)
        assert same(r.ReadFramebuffer(), img) and same(img, plain[0])
        r.Denoise()  # the assembled frame is a frame like any other
        assert r.ReadDenoised().shape == (H, W, 4)


@pytest.mark.parametrize("case", ["offset", "seed", "nee_on", "nee_off"])
def test_accumulate_refusals(P, box, case):
    """Frame A (2 spp, 2 streams), then a PT_FLAG_ACCUMULATE frame that does not continue it: each of the three refusals with its own
    words. A refusal leaves the sums invalid: the frame that would have continued A is refused as well."""
    N = P.native
    acc, nee = N.PT_FLAG_ACCUMULATE, N.PT_FLAG_NEXT_EVENT
    a_flags = nee if case == "nee_off" else 0
    bad, words = {
        "offset": (dict(sample_offset=3, flags=acc), ("sample_offset must be 2",)),
        "seed": (dict(sample_offset=2, flags=acc, seed=7), ("same size, rank, nranks, streams and seed",)),
        "nee_on": (dict(sample_offset=2, flags=acc | nee), ("made without PT_FLAG_NEXT_EVENT",)),
        "nee_off": (dict(sample_offset=2, flags=acc), ("made with PT_FLAG_NEXT_EVENT",)),
    }[case]
    with context(P, box) as r:
        render(P, r, flags=a_flags)
        r.Params = frame(P, **bad)
        refused(P, lambda: r.Render(0.0), N.PT_ERR_INVALID_ARGUMENT, "PT_FLAG_ACCUMULATE", *words)
        r.Params = frame(P, sample_offset=2, flags=acc | a_flags)
        refused(P, lambda: r.Render(0.0), N.PT_ERR_INVALID_ARGUMENT, "needs a previous frame")
        refused(P, r.ReadFramebuffer, N.PT_ERR_NOT_COMMITTED)
        # ... and A again, continued correctly, is the 4-sample frame of a context that was never refused
        render(P, r, flags=a_flags)
        got, st = render(P, r, sample_offset=2, flags=acc | a_flags)
    with context(P, box) as r:
        render(P, r, flags=a_flags)
        want, st_want = render(P, r, sample_offset=2, flags=acc | a_flags)
    assert same(got, want) and st.rays == st_want.rays


@pytest.mark.parametrize("spp", [2, 1])  # 1 spp on 2 streams: the dense template, whose launch bound is read back when it is built
def test_template_across_readback_modes(P, box, spp):
    """The same frame with the queue sizes stored by the kernels, copied per launch, and stored again: the second and third frames start
    from the template the first one built."""
    N = P.native
    with context(P, box) as r:
        if r.GetTuning().readback != 0:
            pytest.skip("no host-mapped pinned memory: pt_tuning.readback = 0 is unsupported here")
        out = []
        for mode in (0, 1, 0):
            r.SetTuning(readback=mode)
            assert r.GetTuning().readback == mode
            img, st = render(P, r, spp=spp)
            out.append((img, int(st.rays), int(st.paths)))
        assert same(out[0][0], out[1][0]) and same(out[0][0], out[2][0])
        assert out[0][1] == out[1][1] == out[2][1] > 0 and out[0][2] == out[1][2] == out[2][2] == W * H * spp


def test_tiles_outlive_frames_of_another_kind(P, box):
    """pt_tiles_device_ptr answers with the last path-traced frame's block after a reference-sphere frame and after a refused frame.
    Stale-looking, and pinned as it is."""
    N = P.native
    with context(P, box) as r:
        ptr, n = C.c_void_p(), C.c_uint64()
        assert N.lib.pt_tiles_device_ptr(r._ctx, C.byref(ptr), C.byref(n)) == N.PT_ERR_NOT_COMMITTED
        render(P, r)
        lay = P.tile_layout(r.Params)
        want = lay.tiles_per_rank * lay.floats_per_tile
        assert r.TilesDevice().__cuda_array_interface__["shape"] == (want,)
        r.Params = P.make_params(W, H, mode=N.PT_REFERENCE_SPHERE)
        r.Render(0.0)
        assert r.TilesDevice().__cuda_array_interface__["shape"] == (want,)
        r.Params = frame(P, spp=0)
        refused(P, lambda: r.Render(0.0), N.PT_ERR_INVALID_ARGUMENT)
        assert r.TilesDevice().__cuda_array_interface__["shape"] == (want,)
