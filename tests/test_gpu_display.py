"""-m gpu: pt_display (docs/SPEC.md §10) on the device against the scalar checker of tests/display_ref/.

The 8-bit image, the 512 histogram words and the info record are compared bit for bit for every curve x {sRGB, LINEAR} x {manual, AUTO,
AUTO with trim}, on frames of 1x1 (a single lane), 7x5 (a partial wave), 65x33 (partial workgroups, a ragged last row) and 256x256 (many
workgroups flushing the same bins), plus one of 1031x517, a size at which the capped grid of the two streaming kernels takes a second
step. The frames are put into the framebuffer through pt_assemble_tiles. Also: sequences of adapting calls, the three sources, what
survives which call, every refusal, and the CLI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import display_checker as dc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32
SHAPES = [(1, 1), (7, 5), (65, 33), (256, 256)]  # (w, h)
CURVES = ["clamp", "reinhard", "aces"]
SOURCES = {"frame": dc.FRAME, "denoised": dc.DENOISED, "temporal": dc.TEMPORAL}
SPECIALS = [0.0, -0.0, -1.5, 1e-40, -1e-40, np.inf, -np.inf, np.nan, 2.0 ** 32, 3e38, 2.0 ** -33]


def assemble(P, r, img):
    """Make `img` ((h, w, 4) float32) the renderer's framebuffer through the public ABI: a tile-major buffer in SPEC §6 slot order,
    pt_assemble_tiles with spp = 1 (the framebuffer is then the buffer times 1.0f). Returns the framebuffer as read back."""
    import torch
    h, w = img.shape[:2]
    p = P.make_params(w, h, spp=1, max_depth=1)
    lay = P.tile_layout(p)
    ts = lay.tile_size
    buf = np.zeros((lay.tiles_per_rank, ts // 8, ts // 8, 8, 8, 4), np.float32)  # tile, block row, block col, row, col
    y, x = np.mgrid[0:h, 0:w]
    tile = (y // ts) * lay.tiles_x + x // ts
    ly, lx = y % ts, x % ts
    buf[tile, ly // 8, lx // 8, ly % 8, lx % 8] = img
    g = torch.from_numpy(buf.reshape(-1)).cuda()
    torch.cuda.synchronize()
    r.Params = p
    r.AssembleTiles(g.data_ptr(), g.numel())
    torch.cuda.synchronize()
    fb = r.ReadFramebuffer()
    finite = np.isfinite(img)
    assert np.array_equal(fb[finite].view(np.uint32), np.ascontiguousarray(img, F32)[finite].view(np.uint32))
    return fb


def hdr_image(seed, w, h, planted=True):
    """Radiance over 28 octaves; with `planted`, every special value in every channel and in alpha (as far as the pixels go)."""
    rng = np.random.default_rng(seed)
    img = np.exp2(rng.uniform(-20.0, 8.0, (h, w, 4))).astype(F32)
    img[..., 3] = rng.uniform(-0.2, 1.2, (h, w)).astype(F32)
    if planted:
        flat = img.reshape(-1, 4)
        where = rng.permutation(len(flat))
        for i, (ch, v) in enumerate((ch, v) for ch in range(4) for v in SPECIALS):
            flat[where[i % len(flat)], ch] = v
    return img


class Mirror:
    """The device and the checker side by side: the checker's adaptation state is carried here, the device's in the context. The first
    call of a Mirror resets the adaptation on both sides: the session's context may have adapted in an earlier test."""

    def __init__(self, P, r):
        self.P, self.r, self.state, self.first = P, r, None, True

    def show(self, ctx, src=None, source="frame", curve="clamp", exposure=0.0, auto=False, white=0.0, key=0.0, adapt=0.0, trim_low=0,
             trim_high=0, linear=False, reset=False):
        """One Display; everything it hands out equals what the checker makes of `src` (default: the framebuffer) bit for bit."""
        r = self.r
        if src is None:
            src = r.ReadFramebuffer()
        h, w = src.shape[:2]
        reset, self.first = reset or self.first, False
        flags = (dc.AUTO if auto else 0) | (dc.LINEAR if linear else 0) | (dc.RESET if reset else 0)
        p = dc.params(SOURCES[source], CURVES.index(curve), exposure, white, key, adapt, trim_low, trim_high, flags)
        want = dc.display(src, p, self.state)
        st = r.Display(source, curve, exposure, auto, white, key, adapt, trim_low, trim_high, linear, reset)
        got, hist, info = r.ReadDisplay(), r.ReadDisplayHistogram(), r.DisplayInfo()
        assert dc.info_tuple(info) == dc.info_tuple(want.info), (ctx, dc.info_tuple(info), dc.info_tuple(want.info))
        bad = np.argwhere(hist != want.histogram)
        assert len(bad) == 0, (ctx, bad[:4].ravel().tolist(), hist[bad[:4].ravel()].tolist(), want.histogram[bad[:4].ravel()].tolist())
        bad = np.argwhere((got != want.image).any(axis=2))
        assert len(bad) == 0, (ctx, len(bad), bad[:3].tolist(), got[tuple(bad[0])].tolist(), want.image[tuple(bad[0])].tolist(),
                               src[tuple(bad[0])].tolist())
        assert st.paths == w * h and st.rays == 0 and st.iterations == 0 and st.node_visits == 0 and st.shade_ms == 0
        assert st.extend_ms >= 0 and st.other_ms > 0 and st.gpu_ms == st.extend_ms + st.other_ms
        self.state = want.state
        return want


def not_committed(P, call):
    with pytest.raises(P.PtException) as e:
        call()
    assert e.value.status == P.native.PT_ERR_NOT_COMMITTED
    return e.value


# ------------------------------------------------------------------------------------------------ bit-identity

@pytest.mark.parametrize("w,h", SHAPES)
def test_every_mode_on_hdr_frames_with_planted_values(P, renderer, w, h):
    fb = assemble(P, renderer, hdr_image(100 + w, w, h))
    m = Mirror(P, renderer)
    for curve in CURVES:
        for linear in (False, True):
            ctx = (w, h, curve, linear)
            m.show(ctx + ("manual",), fb, curve=curve, linear=linear, exposure=0.6, white=3.0)
            m.show(ctx + ("auto",), fb, curve=curve, linear=linear, auto=True, reset=True)
            m.show(ctx + ("trim",), fb, curve=curve, linear=linear, auto=True, reset=True, trim_low=100, trim_high=50, key=0.3, exposure=1.5)
    m.show((w, h, "defaults"), fb)


def test_every_threshold_and_its_neighbours(P, renderer):
    t = dc.table()[1:]
    vals = np.stack([np.nextafter(t, F32(-1)), t, np.nextafter(t, F32(2))], axis=1)  # r, g, b of pixel k - 1
    img = np.zeros((33, 65, 4), F32)
    img.reshape(-1, 4)[:255, :3] = vals
    img.reshape(-1, 4)[255:510, :3] = vals[:, ::-1]
    img[..., 3] = 1.0
    fb = assemble(P, renderer, img)
    want = Mirror(P, renderer).show("thresholds", fb)
    k = np.arange(1, 256)
    px = want.image.reshape(-1, 4)
    assert np.array_equal(px[:255, 0], k - 1) and np.array_equal(px[:255, 1], k) and np.array_equal(px[:255, 2], k)
    # k/255 shows as pt_framebuffer_read_srgb8 shows it
    img = np.zeros((5, 65, 4), F32)
    img.reshape(-1, 4)[:256, :3] = (np.arange(256, dtype=F32) / F32(255.0))[:, None]
    assemble(P, renderer, img)
    Mirror(P, renderer).show("k/255")
    assert np.array_equal(renderer.ReadDisplay()[..., :3], renderer.ReadFramebufferSRGB8()[..., :3])


def test_flat_all_bins_and_black_frames(P, renderer):
    flat = np.empty((256, 256, 4), F32)
    flat[...] = (0.18, 0.18, 0.18, 1.0)
    m = Mirror(P, renderer)
    want = m.show("flat", assemble(P, renderer, flat), auto=True, curve="aces")
    assert np.count_nonzero(want.histogram) == 1 and want.histogram.sum() == 256 * 256
    # one pixel in the middle of every bin, the rest spread over them
    edges = ((np.arange(512, dtype=np.uint32) + 760) << 20).view(F32)
    img = np.empty((33, 65, 4), F32)
    img.reshape(-1, 4)[:, :3] = (edges[np.arange(33 * 65) % 512] * F32(1.03))[:, None]
    img[..., 3] = 0.5
    want = m.show("all bins", assemble(P, renderer, img), auto=True, curve="reinhard", trim_low=10, trim_high=10)
    assert np.all(want.histogram > 0) and want.info.counted == 33 * 65
    # all black: the previous exposure is kept, or 1 without one
    black = np.zeros((7, 5, 4), F32)
    fb = assemble(P, renderer, black)
    want = m.show("black, state", fb, auto=True, adapt=0.5)
    assert want.info.counted == 0 and want.info.adapted == 1 and np.float32(want.info.exposure) == m.state
    want = m.show("black, reset", fb, auto=True, reset=True)
    assert want.info.exposure == 1.0 and want.info.adapted == 0 and m.state == F32(1.0)


def test_a_frame_the_capped_grid_walks_twice(P, renderer):
    """1031 x 517 = 533 027 pixels > 2048 workgroups x 256: the grid-stride loops of the histogram and tone kernels take a second,
    partial step."""
    fb = assemble(P, renderer, hdr_image(7, 1031, 517, planted=False))
    Mirror(P, renderer).show("large", fb, auto=True, curve="aces", trim_high=20)


# ------------------------------------------------------------------------------------------------ adaptation across calls

def test_five_adapting_calls_a_reset_and_a_render_between(P, renderer):
    r = renderer
    m = Mirror(P, r)
    levels = [0.02, 3.0, 40.0, 0.5, 0.004]
    states = []
    for i, level in enumerate(levels):
        img = hdr_image(300 + i, 65, 33, planted=(i == 1))
        with np.errstate(over="ignore"):
            img[..., :3] *= F32(level)
        fb = assemble(P, r, img)
        want = m.show(("sequence", i), fb, auto=True, adapt=0.25, curve="aces", reset=(i == 0 or i == 3))
        assert want.info.adapted == (0 if i in (0, 3) else 1)
        states.append(m.state)
        if i == 1:  # a pt_render drops the displayed results, not the state
            r.Params = P.make_params(720, 640, mode=P.native.PT_REFERENCE_SPHERE)  # (the sphere is around pixel (540, 540))
            r.Render(0.0)
            for read in (r.ReadDisplay, r.DisplayInfo, r.ReadDisplayHistogram):
                not_committed(P, read)
            ptr, n = C.c_void_p(), C.c_uint64()
            assert P.native.lib.pt_display_device_ptr(r._ctx, C.byref(ptr), C.byref(n)) == P.native.PT_ERR_NOT_COMMITTED
            want = m.show("after the render", auto=True, adapt=0.25)
            assert want.info.adapted == 1 and want.info.counted > 0 and m.state != states[-1]
    assert len(set(float(s) for s in states)) == 5
    # a manual call in between neither reads nor writes the state
    before = m.state
    m.show("manual", exposure=2.0)
    assert m.state == before
    assert m.show("adapts from the same state", auto=True, adapt=0.25).info.adapted == 1


# ------------------------------------------------------------------------------------------------ the three sources

def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def test_the_three_sources_and_what_a_display_leaves_alone(P, renderer):
    r = renderer
    w, h = 64, 48
    sd = P.make_scene(P.native.PT_SCENE_CORNELL, 0, 3, w, h)
    r.SetScene(sd)
    r.Params = P.make_params(w, h, spp=1, max_depth=6, seed=21)
    r.Render(0.0)
    m = Mirror(P, r)
    for source in ("denoised", "temporal"):
        e = not_committed(P, lambda: r.Display(source=source))
        assert source[:6] in str(e) or "accumulated" in str(e)
    r.Denoise()
    r.DenoiseTemporal(reset=True)
    r.Params = P.make_params(w, h, spp=1, max_depth=6, seed=22)
    r.Render(0.0)
    r.DenoiseTemporal()
    fb, dn, tm, hl = r.ReadFramebuffer(), r.ReadDenoised(), r.ReadTemporal(), r.ReadHistoryLength()
    assert (hl > 1).any()
    shown = {}
    for source, src in (("frame", fb), ("denoised", dn), ("temporal", tm)):
        m.show(source, src, source=source, curve="aces", auto=True, reset=True, trim_high=10)
        m.show(source + " manual", src, source=source, curve="reinhard", exposure=4.0)
        shown[source] = r.ReadDisplay()
    assert not np.array_equal(shown["frame"], shown["denoised"])
    for got, was in ((r.ReadFramebuffer(), fb), (r.ReadDenoised(), dn), (r.ReadTemporal(), tm), (r.ReadHistoryLength(), hl)):
        assert np.array_equal(bits(got), bits(was))
    # the displayed image survives pt_denoise, pt_denoise_temporal and pt_trace_rays ...
    last, info = r.ReadDisplay(), dc.info_tuple(r.DisplayInfo())
    r.Denoise(iterations=1)
    r.DenoiseTemporal(filter=False)
    r.TraceRays((np.zeros((4, 3), F32), np.tile(np.array([0, 0, -1], F32), (4, 1))))
    assert np.array_equal(r.ReadDisplay(), last) and dc.info_tuple(r.DisplayInfo()) == info
    ptr, n = C.c_void_p(), C.c_uint64()
    assert P.native.lib.pt_display_device_ptr(r._ctx, C.byref(ptr), C.byref(n)) == P.native.PT_OK and ptr.value and n.value == w * h * 4
    # ... and a guides-only denoise leaves no denoised image to display
    r.Denoise(guides_only=True)
    not_committed(P, lambda: r.Display(source="denoised"))
    assert np.array_equal(r.ReadDisplay(), last)


# ------------------------------------------------------------------------------------------------ lifetimes and refusals

def test_not_committed_before_any_frame(P):
    r = P.Renderer(P.Window(8, 8))
    r.Init()
    try:
        r.Params = P.make_params(8, 8)
        for source in SOURCES:
            not_committed(P, lambda: r.Display(source=source))
        for read in (r.ReadDisplay, r.DisplayInfo, r.ReadDisplayHistogram):
            not_committed(P, read)
    finally:
        r.Dispose()


def test_a_refused_call_changes_nothing(P, renderer):
    r, N = renderer, P.native
    fb = assemble(P, r, hdr_image(55, 65, 33))
    m = Mirror(P, r)
    m.show("first", fb, auto=True, curve="aces")
    img, hist, info = r.ReadDisplay(), r.ReadDisplayHistogram(), dc.info_tuple(r.DisplayInfo())
    refused = [
        (dict(exposure=-1.0, auto=True, reset=True), N.PT_ERR_INVALID_ARGUMENT),
        (dict(trim_low=600, trim_high=400, auto=True, reset=True), N.PT_ERR_INVALID_ARGUMENT),
        (dict(adapt=2.0, reset=True), N.PT_ERR_INVALID_ARGUMENT),
        (dict(source="denoised", auto=True, reset=True), N.PT_ERR_NOT_COMMITTED),
        (dict(source="temporal", reset=True), N.PT_ERR_NOT_COMMITTED),
    ]
    for kw, status in refused:
        with pytest.raises(P.PtException) as e:
            r.Display(**kw)
        assert e.value.status == status, kw
        assert np.array_equal(r.ReadDisplay(), img) and np.array_equal(r.ReadDisplayHistogram(), hist)
        assert dc.info_tuple(r.DisplayInfo()) == info
    dp = N.pt_display_params(source=9)
    assert N.lib.pt_display(r._ctx, C.byref(dp), None) == N.PT_ERR_INVALID_ARGUMENT  # (and stats may be NULL)
    assert N.lib.pt_display(r._ctx, None, None) == N.PT_ERR_INVALID_ARGUMENT
    small = (C.c_uint8 * 16)()
    assert N.lib.pt_display_read(r._ctx, small, 16) == N.PT_ERR_INVALID_ARGUMENT
    assert N.lib.pt_display_histogram_read(r._ctx, small, 4) == N.PT_ERR_INVALID_ARGUMENT
    # the next call adapts from the exposure the first one left
    img2 = hdr_image(56, 65, 33)
    with np.errstate(over="ignore"):
        img2[..., :3] *= F32(30.0)
    want = m.show("after the refusals", assemble_keeping(P, r, img2), auto=True, adapt=0.25)
    assert want.info.adapted == 1
    # stats may be NULL on a call that runs
    dp = N.pt_display_params(curve=N.PT_TONE_ACES)
    assert N.lib.pt_display(r._ctx, C.byref(dp), None) == N.PT_OK


def assemble_keeping(P, r, img):
    """assemble(), after checking that it is what drops the displayed results."""
    fb = assemble(P, r, img)
    for read in (r.ReadDisplay, r.DisplayInfo, r.ReadDisplayHistogram):
        not_committed(P, read)
    return fb


# ------------------------------------------------------------------------------------------------ the CLI

def test_cli_display_equals_the_library(P, renderer, tmp_path):
    cli = os.path.join(os.path.dirname(HERE), "host", "cpp", "ptrt_cli")
    assert os.path.exists(cli), "host/cpp/ptrt_cli is built by __graft_entry__.build()"
    w, h, spp = 96, 64, 2
    r = renderer
    r.SetScene(P.make_scene(P.native.PT_SCENE_CORNELL_GLASS, 0, 0x5EED0001, w, h))
    r.Params = P.make_params(w, h, spp=spp, max_depth=8, streams=8)  # the CLI's defaults
    r.Render(0.0)
    m = Mirror(P, r)
    for extra, source in (([], "frame"), (["--denoise", "2"], "denoised")):
        if source == "denoised":
            r.Denoise(iterations=2)
        src = r.ReadDenoised() if source == "denoised" else r.ReadFramebuffer()
        m.show(("cli", source), src, source=source, curve="aces", auto=True, reset=True)
        want = r.ReadDisplay()
        ppm = str(tmp_path / f"{source}.ppm")
        out = subprocess.run([cli, "--scene", "glass", "--size", f"{w}x{h}", "--spp", str(spp), "--display", "aces", "--auto-exposure",
                              "--ppm", ppm] + extra, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        assert "display: exposure" in out.stdout
        with open(ppm, "rb") as f:
            assert f.readline() == b"P6\n" and f.readline().split() == [str(w).encode(), str(h).encode()] and f.readline() == b"255\n"
            assert np.array_equal(np.frombuffer(f.read(), np.uint8).reshape(h, w, 3), want[..., :3]), source
    bad = subprocess.run([cli, "--display", "filmic"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "clamp, reinhard or aces" in bad.stderr
