"""pt_denoise (docs/SPEC.md §8) without a GPU: the scalar checker of tests/denoise_ref/ against float64 numpy and hand-computed guides,
the filter's defining properties, and the API's plumbing (struct layout, C# mirror, argument checks that need no device).

The device is held to the checker bit for bit by tests/test_gpu_denoise.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import denoise_checker as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H3 = np.array([0.0625, 0.25, 0.375, 0.25, 0.0625])


def hit_guides(h, w, ids=None, normal=(0.0, 0.0, 1.0), t=2.0, albedo=(0.5, 0.5, 0.5)):
    g = np.zeros((h, w, 8), np.float32)
    g[..., 0:3], g[..., 3], g[..., 4:7] = normal, t, albedo
    g[..., 7] = (np.zeros((h, w), np.uint32) if ids is None else np.asarray(ids, np.uint32)).view(np.float32)
    return g


def b3_atrous64(img, passes):
    """The plain B3 à-trous blur in float64: taps outside the image skipped, weights renormalised."""
    cur = img.astype(np.float64)
    h, w = cur.shape[:2]
    for i in range(passes):
        s = 1 << i
        acc = np.zeros_like(cur)
        sw = np.zeros((h, w, 1))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                wt = H3[dx + 2] * H3[dy + 2]
                ys, xs = np.arange(h) + dy * s, np.arange(w) + dx * s
                vy, vx = (ys >= 0) & (ys < h), (xs >= 0) & (xs < w)
                m = vy[:, None] & vx[None, :]
                src = cur[np.clip(ys, 0, h - 1)][:, np.clip(xs, 0, w - 1)]
                acc += np.where(m[..., None], wt * src, 0.0)
                sw += np.where(m[..., None], wt, 0.0)
        cur = np.concatenate([acc[..., :3] / sw, img[..., 3:4].astype(np.float64)], axis=2)
    return cur


def test_checker_builds():
    dc.build()
    assert os.path.exists(os.path.join(dc.DIR, "libdenoise_ref.so"))
    it, sc, sn, sz, sa = dc.defaults()
    assert 1 <= it <= 8 and min(sc, sn, sz, sa) > 0


@pytest.mark.parametrize("passes", [1, 3, 5, 8])
def test_no_edge_stops_is_the_b3_blur(passes):
    rng = np.random.default_rng(passes)
    img = rng.uniform(0, 1, (23, 37, 4)).astype(np.float32)
    out = dc.filter(img, hit_guides(23, 37, rng.integers(0, 5, (23, 37))), dc.params(passes, flags=dc.NO_EDGE_STOPS))
    ref = b3_atrous64(img, passes)
    assert np.abs(out.astype(np.float64) - ref).max() < 1e-6
    assert np.array_equal(out[..., 3], img[..., 3])  # alpha is copied


@pytest.mark.parametrize("passes", [1, 5])
@pytest.mark.parametrize("value", [0.5, 1.0, 4.0, 0.3, 7.25])
def test_constant_image_stays_constant(value, passes):
    """Whatever the guides, a constant colour comes back to within rounding. A power of two scales every partial sum exactly, so sc equals
    value * sw and only sc * (1/sw) rounds: at most 2 ulp per pass. Any other value also rounds its 25 fma partial sums: at most 25/2 ulp
    per pass (the bound of the sum)."""
    rng = np.random.default_rng(1)
    h, w = 40, 50
    g = hit_guides(h, w, rng.integers(0, 3, (h, w)))
    n = rng.normal(size=(h, w, 3)).astype(np.float32)
    g[..., 0:3] = n / np.linalg.norm(n, axis=2, keepdims=True)
    g[..., 3] = rng.uniform(1, 3, (h, w))
    g[..., 4:7] = rng.uniform(0, 1, (h, w, 3))
    img = np.full((h, w, 4), value, np.float32)
    out = dc.filter(img, g, dc.params(passes))
    ulp = np.spacing(np.float32(value))
    per_pass = 2.0 if np.log2(value) == int(np.log2(value)) else 12.5
    assert np.abs(out[..., :3] - np.float32(value)).max() <= per_pass * passes * ulp


def test_step_edge_survives_with_guides_only():
    """A colour step along a geometric edge (normal, depth, albedo and id change there) survives 5 passes of the guided filter and is
    smeared by the plain blur: the guides are what keeps it."""
    h, w = 32, 64
    rng = np.random.default_rng(3)
    img = np.zeros((h, w, 4), np.float32)
    img[:, :32, :3], img[:, 32:, :3], img[..., 3] = 0.1, 0.9, 1.0
    img[..., :3] += rng.normal(0, 0.01, (h, w, 3)).astype(np.float32)
    g = hit_guides(h, w, np.where(np.arange(w) < 32, 0, 1)[None, :].repeat(h, 0))
    g[:, 32:, 0:3] = (1.0, 0.0, 0.0)
    g[:, 32:, 3] = 3.0
    g[:, 32:, 4:7] = 0.9
    guided = dc.filter(img, g, dc.params(5))
    blurred = dc.filter(img, g, dc.params(5, flags=dc.NO_EDGE_STOPS))
    assert abs(guided[:, 31, :3].mean() - 0.1) < 0.01 and abs(guided[:, 32, :3].mean() - 0.9) < 0.01
    assert blurred[:, 31, :3].mean() > 0.3 and blurred[:, 32, :3].mean() < 0.7
    assert guided[:, 4:28, :3].std() < img[:, 4:28, :3].std() / 3  # and the flat sides are still smoothed


def test_misses_are_kept_apart_from_hits():
    """A tap where exactly one of p, q is a miss is skipped: the sky does not bleed into geometry nor geometry into the sky."""
    h, w = 16, 16
    g = hit_guides(h, w)
    g[:, 8:, 0:4] = (0.0, 0.0, 0.0, np.inf)
    g[:, 8:, 4:8] = 0.0
    g[:, 8:, 7] = np.array([dc.MISS], np.uint32).view(np.float32)[0]
    img = np.ones((h, w, 4), np.float32)
    img[:, 8:, :3] = 5.0
    for flags in (0, dc.NO_EDGE_STOPS):
        out = dc.filter(img, g, dc.params(4, flags=flags))
        assert np.abs(out[:, :8, :3] - 1.0).max() < 1e-6 and np.abs(out[:, 8:, :3] - 5.0).max() < 1e-5, flags


def test_guides_of_a_tiny_scene(P, pto):
    """Hand-built scene: a triangle wound away from the camera (its normal is flipped to face the ray), a sphere, sky. Normals, depths,
    albedos and ids against float64 geometry of the same camera rays."""
    N = P.native
    w, h = 12, 8
    sd = P.SceneData()
    sd.verts = np.array([[-4.0, -4.0, -2.0, -4.0, 4.0, -2.0, 0.0, -4.0, -2.0]], np.float32)  # cross(e1, e2) = (0, 0, +32): faces +z
    sd.verts = sd.verts[:, [0, 1, 2, 6, 7, 8, 3, 4, 5]]  # swap v1, v2: ng = (0, 0, -1), away from the camera
    sd.tri_mat = np.array([0], np.uint32)
    sd.spheres = np.array([[0.6, 0.0, -3.0, 0.5]], np.float32)
    sd.sph_mat = np.array([1], np.uint32)
    sd.mats = np.zeros(2, P.MATERIAL_DTYPE)
    sd.mats["albedo"] = [(0.25, 0.5, 0.75), (0.9, 0.1, 0.2)]
    sd.mats[1]["kind"] = N.PT_METAL
    cam = N.pt_camera()
    cam.origin[:] = (0.0, 0.0, 0.0)
    cam.forward[:], cam.right[:], cam.up[:] = (0.0, 0.0, -1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)
    cam.scale, cam.cx, cam.cy, cam.jitter = 2.0 / h, w / h, 1.0, 1  # jitter on: the guides must ignore it
    sd.cam = cam
    g = dc.guides(pto, pto.Scene(sd), w, h)
    ids = g[..., 7].view(np.uint32)
    assert {0, 1, dc.MISS} == set(np.unique(ids).tolist())
    for y in range(h):
        for x in range(w):
            o, d = pto.camera_ray(unjittered(cam), x, y)
            d64 = d.astype(np.float64)
            if ids[y, x] == 0:
                t = -2.0 / d64[2]
                assert np.allclose(g[y, x, 0:3], (0, 0, 1)) and abs(g[y, x, 3] - t) < 1e-5 * t
                assert np.allclose(g[y, x, 4:7], (0.25, 0.5, 0.75))
            elif ids[y, x] == 1:
                c = np.array([0.6, 0.0, -3.0])
                b = np.dot(-c, d64)
                t = -b - np.sqrt(b * b - (np.dot(c, c) - 0.25))
                n = (t * d64 - c) / 0.5
                assert abs(g[y, x, 3] - t) < 1e-5 * t and np.abs(g[y, x, 0:3] - n).max() < 1e-4 and np.dot(n, d64) < 0
                assert np.allclose(g[y, x, 4:7], (0.9, 0.1, 0.2))
            else:
                assert np.isinf(g[y, x, 3]) and not g[y, x, :3].any() and not g[y, x, 4:7].any()


def unjittered(cam):
    c = type(cam)()
    C.memmove(C.byref(c), C.byref(cam), C.sizeof(cam))
    c.jitter = 0
    return c


def test_params_struct_and_csharp_mirror(P):
    N = P.native
    assert C.sizeof(N.pt_denoise_params) == 32 == C.sizeof(dc.dr_params)
    assert [f[0] for f in N.pt_denoise_params._fields_] == [f[0] for f in dc.dr_params._fields_]
    hdr = open(os.path.join(ROOT, "include", "ptrt.h")).read()
    body = re.search(r"typedef struct pt_denoise_params \{(.*?)\} pt_denoise_params;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        m = re.match(r"\s*(\w+)\s+(.*)$", decl, re.S)
        if m:
            for item in m.group(2).split(","):
                am = re.match(r"\s*(\w+)\s*(?:\[(\d+)\])?\s*$", item)
                fields.append(({"uint32_t": "uint", "float": "float"}[m.group(1)], am.group(1), int(am.group(2) or 0)))
    cs = open(os.path.join(ROOT, "host", "csharp", "PtrtNative.cs")).read()
    cbody = re.search(r"struct PtDenoiseParams\s*\{(.*?)\}", cs, re.S).group(1)
    cfields = [(m.group(2), m.group(3), int(m.group(4) or 0))
               for m in re.finditer(r"public\s+(fixed\s+)?(\w+)\s+(\w+)(?:\[(\d+)\])?\s*;", cbody)]
    assert fields == cfields, (fields, cfields)
    assert [f[1] for f in fields] == [f[0] for f in N.pt_denoise_params._fields_]
    assert "PtDenoiseParams* dp" in cs and re.search(r"enum PtDenoiseFlags : uint \{ GuidesOnly = 1, NoEdgeStops = 2 \}", cs)


def test_argument_checks_without_a_device(P):
    N, lib = P.native, P.native.lib

    def err():
        return lib.pt_last_error(None).decode()

    dp = N.pt_denoise_params()
    assert lib.pt_denoise(None, None, None, None) == N.PT_ERR_INVALID_ARGUMENT and "dp is NULL" in err()
    assert lib.pt_denoise(None, None, C.byref(dp), None) == N.PT_ERR_INVALID_ARGUMENT and "NULL context" in err()
    for field, value, what in (("flags", 4, "flag"), ("iterations", 9, "iterations"), ("sigma_color", -1.0, "sigma_color"),
                               ("sigma_normal", float("nan"), "sigma_normal"), ("sigma_depth", float("inf"), "sigma_depth"),
                               ("sigma_albedo", -0.0 - 1e-30, "sigma_albedo")):
        bad = N.pt_denoise_params()
        setattr(bad, field, value)
        assert lib.pt_denoise(None, None, C.byref(bad), None) == N.PT_ERR_INVALID_ARGUMENT and what in err(), (field, err())
    ok = N.pt_denoise_params(8, 1.0, 0.5, 0.25, 0.125, N.PT_DENOISE_GUIDES_ONLY | N.PT_DENOISE_NO_EDGE_STOPS)
    assert lib.pt_denoise(None, None, C.byref(ok), None) == N.PT_ERR_INVALID_ARGUMENT and "NULL context" in err()
    # a detached scene: without a context the call is refused as a NULL context
    s = C.c_void_p()
    assert lib.pt_scene_create(None, C.byref(s)) == 0
    try:
        assert lib.pt_denoise(None, s, C.byref(ok), None) == N.PT_ERR_INVALID_ARGUMENT
    finally:
        lib.pt_scene_destroy(s)
    buf = np.zeros(8, np.float32)
    ptr, n = C.c_void_p(), C.c_uint64()
    assert lib.pt_denoised_read(None, buf.ctypes.data, 8) == N.PT_ERR_INVALID_ARGUMENT
    assert lib.pt_guides_read(None, buf.ctypes.data, 8) == N.PT_ERR_INVALID_ARGUMENT
    assert lib.pt_denoised_device_ptr(None, C.byref(ptr), C.byref(n)) == N.PT_ERR_INVALID_ARGUMENT
