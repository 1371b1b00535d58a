"""-m gpu: pt_denoise (docs/SPEC.md §8) on the device against float64 (tests/denoise64.py), not only against the f32 checker.

The device's guide buffers against guides64 (every layout, both builders, generator and adversarial scenes); the device's filter pass by
pass against atrous_pass64 and its derived bound, on rendered frames and on synthetic colour fields fed through the public ABI
(pt_assemble_tiles of a tile-major buffer with spp = 1 makes the framebuffer exactly that buffer); the σ grid on the device; invariance
under a power-of-two scale of the scene; and the 8-bit read-backs of assembled frames against SPEC §1's unorm8 and the float64 sRGB table."""
import dataclasses

import numpy as np
import pytest

import adversarial_scenes as adv
import denoise64 as d64
import denoise_checker as dc
from trace_support import LAYOUTS

pytestmark = pytest.mark.gpu

FLT_MAX = d64.FLT_MAX
SIGMA_GRID = [2.0 ** -140, 2.0 ** -126, 2.0 ** -60, 2.0 ** -8, 0.3, 1.0, 2.0 ** 8, 3e19, 2.0 ** 60, FLT_MAX]
W, H = 48, 32


def sky_scene(P, w, h):
    """test_gpu_denoise.py's sky scene: C4 seen from further back, so that the sky shows around the open box."""
    sd = P.make_scene(P.native.PT_SCENE_CORNELL_GLASS, 0, 3, w, h)
    cam = type(sd.cam)()
    cam.origin[:] = (0.3, 0.2, 4.5)
    f = np.array([-0.05, -0.03, -1.0]); f /= np.linalg.norm(f)
    r = np.cross(f, [0.0, 1.0, 0.0]); r /= np.linalg.norm(r)
    u = np.cross(r, f)
    cam.forward[:], cam.right[:], cam.up[:] = f.tolist(), (r * 0.3).tolist(), (u * 0.3).tolist()
    cam.scale, cam.cx, cam.cy, cam.jitter = 2.0 / h, w / h, 1.0, 1
    return dataclasses.replace(sd, cam=cam, sky=np.array([0.3, 0.4, 0.6], np.float32))


def scenes(P, w=W, h=H):
    N = P.native
    cornell = P.make_scene(N.PT_SCENE_CORNELL, 0, 3, w, h)
    return {"cornell": cornell, "sky": sky_scene(P, w, h), "tess": P.make_scene(N.PT_SCENE_CORNELL_TESS, 3000, 3, w, h),
            "layers": adv.stacked_layers(w, h), "duplicates": adv.duplicates(w, h)[0], "axis": adv.axis_camera(cornell, w + 1, h + 1),
            "floor": adv.floor_camera(cornell, w + 1, h + 1), "spheres64": adv.sphere_list(64, w, h),
            "inside_sphere": adv.sphere_list(8, w, h, camera_inside=True)}


def size_of(name):
    return (W + 1, H + 1) if name in ("axis", "floor") else (W, H)


def assemble(P, r, img):
    """Make `img` ((h, w, 4) float32) the renderer's framebuffer through the public ABI: a tile-major buffer in SPEC §6 slot order,
    pt_assemble_tiles with spp = 1 (the framebuffer is then exactly the buffer)."""
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
    assert np.array_equal(fb.view(np.uint32), np.ascontiguousarray(img, np.float32).view(np.uint32))
    return fb


def device_pass_by_pass(P, r, sd, n, ctx, **kw):
    """Pass i's input is the device's own output after i passes (Denoise(iterations=i); the framebuffer for i = 0); the device's pass
    i + 1 output must be finite and within the float64 bound. The device's guides and image also equal the checker's bit for bit."""
    prm = d64.resolve64(**kw)
    fb = r.ReadFramebuffer()
    cur, g, worst = fb, None, 0.0
    for i in range(n):
        r.Denoise(iterations=i + 1, **kw)
        out, gi = r.ReadDenoised(), r.ReadGuides()
        if g is None:
            g = gi
        assert np.array_equal(gi.view(np.uint32), g.view(np.uint32))
        ratio, at = d64.pass_error(out, cur, g, i, prm)
        assert ratio <= 1.0, (ctx, kw, i, ratio, at)
        worst = max(worst, ratio)
        cur = out
    want = dc.filter(fb, g, dc.params(n, **kw))
    assert np.array_equal(cur.view(np.uint32), want.view(np.uint32)), (ctx, kw)
    return worst, g


def test_guides_against_float64(P, pto, renderer):
    """ReadGuides() against guides64 on every layout and both builders: ids agree except where float64 cannot settle them, normal and t
    within the derived bound on agreeing hits, albedo exact, misses exact."""
    N = P.native
    for name, sd in scenes(P).items():
        w, h = size_of(name)
        ref = d64.guides64(pto, sd, w, h)
        for width in LAYOUTS:
            for build in (0, N.PT_BVH_BUILD_LBVH):
                renderer.SetScene(sd, width | build)
                renderer.Params = P.make_params(w, h, spp=1, max_depth=1)
                renderer.Render(0.0)
                renderer.Denoise(guides_only=True)
                agree, _, _ = d64.compare_guides(renderer.ReadGuides(), ref, w, h)
                assert agree >= 0.95 * w * h, (name, width, build, agree)


def test_rendered_frames_pass_by_pass(P, pto, renderer):
    """4-spp frames of the generator and adversarial scenes, 8 passes, each pass of the device against the float64 pass."""
    worst = {}
    for name, sd in scenes(P).items():
        w, h = size_of(name)
        renderer.SetScene(sd, 0)
        renderer.Params = P.make_params(w, h, spp=4, max_depth=6)
        renderer.Render(0.0)
        worst[name], _ = device_pass_by_pass(P, renderer, sd, 8, name)
        worst[name + " σ"], _ = device_pass_by_pass(P, renderer, sd, 3, name, sigma_color=0.3, sigma_normal=0.7, sigma_depth=0.02,
                                                    sigma_albedo=0.1)
    print("worst error / bound per scene:", {k: round(v, 3) for k, v in worst.items()})


def synthetic(shape, seed, hdr=False):
    rng = np.random.default_rng(seed)
    h, w = shape
    img = np.zeros((h, w, 4), np.float32)
    img[..., :3] = rng.uniform(0, 1, (h, w, 3))
    img[..., 3] = rng.uniform(0, 1, (h, w))
    if hdr:
        img[..., :3] *= (2.0 ** rng.uniform(-30, 100, (h, w, 1))).astype(np.float32)
        img[rng.uniform(size=(h, w)) < 0.1, :3] = 0.0
    img[rng.uniform(size=(h, w)) < 0.02, :3] = 1e6  # fireflies
    return img


@pytest.mark.parametrize("w,h", [(1, 1), (29, 1), (1, 23), (67, 45)])
def test_synthetic_fields_pass_by_pass(P, renderer, w, h):
    """Synthetic colour fields (LDR and HDR up to 2^100, fireflies, zeros) over the sky scene's guides, through pt_assemble_tiles: every
    pass of 8 against float64."""
    sd = sky_scene(P, w, h)
    renderer.SetScene(sd, 0)
    for seed, hdr in ((1, False), (2, True)):
        assemble(P, renderer, synthetic((h, w), seed, hdr))
        device_pass_by_pass(P, renderer, sd, 8, (w, h, hdr))


def test_one_pass_at_1080p(P, renderer):
    w, h = 1920, 1080
    sd = sky_scene(P, w, h)
    renderer.SetScene(sd, 0)
    assemble(P, renderer, synthetic((h, w), 3))
    device_pass_by_pass(P, renderer, sd, 1, "1080p")


@pytest.mark.parametrize("which", ["sigma_color", "sigma_normal", "sigma_depth", "sigma_albedo"])
def test_finite_over_the_sigma_grid(P, renderer, which):
    """Each σ over its log grid on the device, 8 passes: finite and within the float64 bound (the device is also the checker, bit for
    bit), on an LDR and an HDR field."""
    w, h = 37, 29
    sd = sky_scene(P, w, h)
    renderer.SetScene(sd, 0)
    for seed, hdr in ((4, False), (5, True)):
        assemble(P, renderer, synthetic((h, w), seed, hdr))
        for v in SIGMA_GRID:
            device_pass_by_pass(P, renderer, sd, 8, (which, v, hdr), **{which: v})


def test_finite_at_the_corners_of_the_issue(P, renderer):
    """The accepted parameter sets that made every pixel NaN: each is finite on the device now, and within the float64 bound."""
    w, h = 16, 16
    sd = P.make_scene(P.native.PT_SCENE_CORNELL, 0, 3, w, h)
    renderer.SetScene(sd, 0)
    flat = np.full((h, w, 4), 0.5, np.float32)
    hdr = flat.copy()
    hdr[..., :3] = np.random.default_rng(6).uniform(0, 1, (h, w, 3)) * 1e20
    for img, kw in ((flat, dict(sigma_color=2e-20)), (flat, dict(sigma_color=1e-18)), (flat, dict(sigma_normal=2.0 ** -126)),
                    (flat, dict(sigma_albedo=2e-20)), (hdr, dict(sigma_color=1e30))):
        assemble(P, renderer, img)
        device_pass_by_pass(P, renderer, sd, 8, kw, **kw)
    small = adv.scaled(sd, -30)  # the depths of a 2^-30-scaled scene with σ_z = 1e-30: 1/(σ_z·t) overflows
    renderer.SetScene(small, 0)
    assemble(P, renderer, flat)
    device_pass_by_pass(P, renderer, small, 4, "2^-30", sigma_depth=1e-30)


SCALED = [pytest.param(name, k, marks=pytest.mark.xfail(strict=True, reason="SPEC §5 normalize: |e1 x e2|^2 of the small tessellated "
                                                         "triangles is subnormal at 2^-30, so the normal's bits change (out of scope here)"))
          if (name, k) == ("tess", -30) else (name, k) for name in ("cornell", "sky", "spheres64", "tess") for k in (-30, -8, 8, 30)]


@pytest.mark.parametrize("name,k", SCALED)
def test_power_of_two_scale(P, renderer, name, k):
    """All lengths times 2^k: the guides' t scale exactly, the normals, albedos and ids are identical, x_z is invariant, so the denoised
    image of the same framebuffer is bit-identical to the unscaled one. (The stacked layers are left out: their widest layer is 2^60
    across, and its |e1 x e2|^2 overflows at 2^30.)"""
    w, h = W, H
    sd = scenes(P)[name]
    img = synthetic((h, w), 7)
    out = []
    for s in (sd, adv.scaled(sd, k)):
        renderer.SetScene(s, 0)
        assemble(P, renderer, img)
        renderer.Denoise(iterations=5)
        out.append((renderer.ReadGuides(), renderer.ReadDenoised()))
    (g0, d0), (g1, d1) = out
    assert np.array_equal(g1[..., 3], (g0[..., 3] * np.float32(2.0 ** k)).astype(np.float32))
    assert np.array_equal(g1[..., :3].view(np.uint32), g0[..., :3].view(np.uint32)), int((g1[..., :3] != g0[..., :3]).any(-1).sum())
    assert np.array_equal(g1[..., 4:].view(np.uint32), g0[..., 4:].view(np.uint32))
    assert np.array_equal(d1.view(np.uint32), d0.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------ 8-bit read-backs
def unorm8(v):
    """SPEC §1 in f32: floor(min(max(c, 0), 1) * 255.0f + 0.5f), NaN -> 0."""
    v = np.asarray(v, np.float32)
    c = np.where(np.isnan(v), np.float32(0), np.minimum(np.maximum(v, np.float32(0)), np.float32(1))).astype(np.float32)
    return np.floor(c * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)


def srgb8_table():
    """round(255 * srgb_oetf(q / 255)) for every 8-bit q, in float64."""
    q = np.arange(256) / 255.0
    e = np.where(q <= 0.0031308, 12.92 * q, 1.055 * q ** (1 / 2.4) - 0.055)
    return np.floor(255.0 * e + 0.5).astype(np.uint8)


def test_rgba8_and_srgb8_of_an_assembled_frame(P, renderer):
    """pt_framebuffer_read_rgba8 and _srgb8 of an assembled frame against §1's unorm8 and the float64 sRGB table, on every k/255 and its
    two f32 neighbours, 0, -0, negatives, subnormals, 1 and the next float above it, 1e30, +-inf and NaN, in every channel."""
    f32 = np.float32
    k = (np.arange(256) / 255.0).astype(f32)
    vals = np.concatenate([k, np.nextafter(k, f32(-1)), np.nextafter(k, f32(2)),
                           np.array([0.0, -0.0, -1.0, -1e-30, -1e30, 1e-45, 1e-40, 2.0 ** -126, 1.0, np.nextafter(f32(1), f32(2)), 1.5,
                                     1e30, np.inf, -np.inf, np.nan, 0.5 / 255, np.nextafter(f32(0.5 / 255), f32(0))], f32)]).astype(f32)
    n = len(vals)
    w = 37
    h = -(-n // w)
    flat = np.resize(vals, h * w * 4).astype(f32)
    img = np.stack([flat[: h * w], np.roll(flat, 7)[: h * w], np.roll(flat, 19)[: h * w], np.roll(flat, 101)[: h * w]], -1).reshape(h, w, 4)
    sd = P.make_scene(P.native.PT_SCENE_CORNELL, 0, 3, w, h)
    renderer.SetScene(sd, 0)
    assemble(P, renderer, img)
    want = unorm8(img)
    assert want[..., 0][np.isnan(img[..., 0])].max(initial=0) == 0 and (unorm8(k) == np.arange(256)).all()
    got = renderer.ReadFramebufferRGBA8()
    bad = np.argwhere(got != want)
    assert len(bad) == 0, [(img[tuple(b)], got[tuple(b)], want[tuple(b)]) for b in bad[:5]]
    lut = srgb8_table()
    srgb = renderer.ReadFramebufferSRGB8()
    assert np.array_equal(srgb[..., :3], lut[want[..., :3]]) and np.array_equal(srgb[..., 3], want[..., 3])
