"""ctypes binding of tests/env_ref/libenv_ref.so — the scalar restatement of docs/SPEC.md §11 (environment-map lighting, with the §5
loop and §7 light sample around it) that the environment tests check the product against — and the maps and scenes those tests share.
Test infrastructure only, like oracle/pto.py."""
import ctypes as C
import dataclasses

import numpy as np

import ref_lib

NEE, NO_JACOBIAN, NO_MIS, NO_PSEL, SAMPLED_TEXEL = 1, 2, 4, 8, 16


class er_stats(C.Structure):
    _fields_ = [("ext_rays", C.c_uint64), ("shadow_rays", C.c_uint64), ("paths", C.c_uint64), ("n_lights", C.c_uint64),
                ("lit", C.c_uint32), ("pad", C.c_uint32)]


_f3, _u2 = C.c_float * 3, C.c_uint32 * 2
SYMBOLS = {
    "er_decode": (None, [C.c_float, C.c_float, _f3]),
    "er_encode": (C.c_float, [_f3, C.c_uint32, _u2]),
    "er_texel_solid_angle": (C.c_double, [C.c_uint32, C.c_uint32, C.c_uint32]),
    "er_table": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    "er_render": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(er_stats)]),
}


def build():
    return ref_lib.load("env_ref", "libenv_ref.so", SYMBOLS)


def decode(u, v):
    d = _f3()
    build().er_decode(u, v, d)
    return np.array(d[:], np.float32)


def encode(d, n):
    """(column i, row j, s) of direction d on the n x n map."""
    ij = _u2()
    s = build().er_encode(_f3(*[float(x) for x in d]), n, ij)
    return int(ij[0]), int(ij[1]), float(s)


def texel_solid_angle(i, j, n):
    return float(build().er_texel_solid_angle(i, j, n))


def table(rgb):
    """(texels4 n x n x 4, mcdf n, ccdf n x n, lit, total) of the map rgb (n x n x 3), as §11 builds it."""
    a = np.ascontiguousarray(rgb, np.float32)
    n = a.shape[0]
    tex, mcdf, ccdf = np.zeros((n, n, 4), np.float32), np.zeros(n, np.float32), np.zeros((n, n), np.float32)
    total = C.c_double()
    lit = build().er_table(a.ctypes.data, n, tex.ctypes.data, mcdf.ctypes.data, ccdf.ctypes.data, C.byref(total))
    assert lit >= 0
    return tex, mcdf, ccdf, lit, total.value


def render(pto, scene, params, env=None, flags=0, with_sq=False, threads=0):
    """(rgba float32 HxWx4, er_stats, per-pixel sums of squared sample radiance HxWx3 float64 or None). `env`: n x n x 3 or None."""
    lib = build()
    p = pto.pto_params()
    C.memmove(C.byref(p), C.byref(params), C.sizeof(pto.pto_params))
    out = np.zeros((p.height, p.width, 4), np.float32)
    sq = np.zeros((p.height, p.width, 3), np.float64) if with_sq else None
    e = None if env is None else np.ascontiguousarray(env, np.float32)
    st = er_stats()
    rc = lib.er_render(C.addressof(scene.c), C.addressof(p), None if e is None else e.ctypes.data, 0 if e is None else e.shape[0], flags,
                       threads, out.ctypes.data, None if sq is None else sq.ctypes.data, C.byref(st))
    if rc != 0:
        raise RuntimeError(f"er_render failed: {rc}")
    return out, st, sq


# ------------------------------------------------------------------------------------------------------------------------ maps and scenes
SUN_DIR = (0.35, 0.8, 0.5)


def sun_sky(P, n=64):
    """A dim blue sky with a sun of 18 degrees radius (cos 0.95) that carries most of the map's power: wide and dim enough for the
    plain estimator's 2048-sample mean to be near normal (a 6-degree sun of ten times the radiance leaves it a handful of hits per pixel
    block and no usable variance estimate), small and bright enough for light sampling to cut the variance several times."""
    return P.sun_sky_environment(n, SUN_DIR, (40.0, 36.0, 30.0), 0.95, (0.3, 0.4, 0.6))


def distinct(n):
    """Every texel its own colour."""
    k = np.arange(n * n, dtype=np.float32).reshape(n, n)
    return np.stack([1.0 + k, 0.5 + 2.0 * k, 0.25 + 3.0 * k], -1).astype(np.float32)


def scene(P, name, w, h, detail=500):
    """soup: C3 (`detail` triangles) without its constant sky; cornell / glass: C1 / C2, whose open front lets the environment in."""
    N = P.native
    if name == "soup":
        return dataclasses.replace(P.make_scene(N.PT_SCENE_TRIANGLE_SOUP, detail, 3, w, h), sky=np.zeros(3, np.float32))
    return P.make_scene(N.PT_SCENE_CORNELL if name == "cornell" else N.PT_SCENE_CORNELL_GLASS, 0, 3, w, h)


def one_triangle_scene(P, w, h):
    """One small grey triangle in front of a jitter-free camera at the origin looking down -z. Pixel (w/2, h/2) looks exactly along -z
    (an axis of the map), its column and row have d.x = 0 / d.y = 0 (the lower half's fold lines, where sgn flips), and the field of
    view is wide enough for many texels."""
    sd = P.make_scene(P.native.PT_SCENE_CORNELL, 0, 3, w, h)
    cam = P.native.pt_camera()
    cam.origin[:] = (0.0, 0.0, 0.0)
    cam.forward[:] = (0.0, 0.0, -1.0)
    cam.right[:] = (1.0, 0.0, 0.0)
    cam.up[:] = (0.0, 1.0, 0.0)
    cam.scale, cam.cx, cam.cy, cam.jitter = 0.125, (w // 2 + 0.5) * 0.125, (h // 2 + 0.5) * 0.125, 0
    mats = np.zeros(1, sd.mats.dtype)
    mats[0]["kind"], mats[0]["albedo"], mats[0]["ior"] = 0, (0.6, 0.6, 0.6), 1.0
    verts = np.array([[0.2, 0.1, -1.0, 0.5, 0.1, -1.0, 0.3, 0.4, -1.2]], np.float32)
    return dataclasses.replace(sd, verts=verts, tri_mat=np.zeros(1, np.uint32), spheres=np.zeros((0, 4), np.float32),
                               sph_mat=np.zeros(0, np.uint32), mats=mats, cam=cam, sky=np.zeros(3, np.float32))
