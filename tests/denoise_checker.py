"""ctypes binding of tests/denoise_ref/libdenoise_ref.so — the scalar restatement of docs/SPEC.md §8 (pt_denoise) that the denoiser tests
check the device against. Test infrastructure only, like oracle/pto.py; `build()` runs its Makefile."""
import ctypes as C
import os

import numpy as np

import ref_lib

DIR = os.path.join(ref_lib.HERE, "denoise_ref")
GUIDES_ONLY, NO_EDGE_STOPS = 1, 2
MISS = 0xFFFFFFFF
# dr_pass variants: §8.2 as written, then the deliberately wrong ones of the negative controls
SPEC, SIGMA_C_FIXED, XZ_NO_STEP, D_LINEAR, WRONG_TAP, NO_MISS_SKIP = range(6)


class dr_params(C.Structure):
    _fields_ = [("iterations", C.c_uint32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float),
                ("sigma_albedo", C.c_float), ("flags", C.c_uint32), ("pad", C.c_uint32 * 2)]


assert C.sizeof(dr_params) == 32


# name -> (restype, argtypes): the entry points of denoise_ref.c
SYMBOLS = {
    "dr_guides": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "dr_filter": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(dr_params), C.c_void_p]),
    "dr_pass": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(dr_params), C.c_uint32, C.c_int, C.c_void_p]),
    "dr_resolve": (C.c_int, [C.POINTER(dr_params), C.POINTER(dr_params)]),
}


def build():
    """The checker, made (incrementally) and loaded on the first call of a process."""
    return ref_lib.load("denoise_ref", "libdenoise_ref.so", SYMBOLS)


def params(iterations=0, sigma_color=0.0, sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0, flags=0):
    return dr_params(iterations, sigma_color, sigma_normal, sigma_depth, sigma_albedo, flags)


def defaults():
    """The §8.2 defaults the checker restates (iterations, sigma_color, sigma_normal, sigma_depth, sigma_albedo)."""
    out = dr_params()
    assert build().dr_resolve(C.byref(params()), C.byref(out)) > 0
    return out.iterations, out.sigma_color, out.sigma_normal, out.sigma_depth, out.sigma_albedo


def guides(pto, scene, w, h):
    """(h, w, 8) float32: g0 = (n, t), g1 = (albedo, prim id bits) of §8.1. `scene`: a pto.Scene (brute force or with a blob)."""
    g = np.zeros((h, w, 8), np.float32)
    assert build().dr_guides(C.addressof(scene.c), w, h, g.ctypes.data) == 0
    return g


def filter(rgba, g8, p=None):
    """§8.2 over an (h, w, 4) float32 image with (h, w, 8) guides; returns the filtered (h, w, 4) image (the input for GUIDES_ONLY)."""
    rgba = np.ascontiguousarray(rgba, np.float32)
    g8 = np.ascontiguousarray(g8, np.float32)
    h, w = rgba.shape[:2]
    assert g8.shape == (h, w, 8)
    out = np.zeros_like(rgba)
    n = build().dr_filter(rgba.ctypes.data, g8.ctypes.data, w, h, C.byref(p if p is not None else params()), out.ctypes.data)
    if n < 0:
        raise ValueError(f"dr_filter refused the parameters ({n})")
    return out if n > 0 else rgba.copy()


def one_pass(rgba, g8, i, p=None, variant=SPEC):
    """Pass i (0-based, step 2^i) of §8.2 alone over an (h, w, 4) float32 image, or one of the wrong variants (negative controls)."""
    rgba = np.ascontiguousarray(rgba, np.float32)
    g8 = np.ascontiguousarray(g8, np.float32)
    h, w = rgba.shape[:2]
    assert g8.shape == (h, w, 8)
    out = np.zeros_like(rgba)
    if build().dr_pass(rgba.ctypes.data, g8.ctypes.data, w, h, C.byref(p if p is not None else params()), i, variant, out.ctypes.data):
        raise ValueError("dr_pass refused the parameters")
    return out


def denoise(pto, scene, rgba, p=None):
    """(guides, denoised image) of §8 for a framebuffer `rgba` rendered on `scene`."""
    h, w = rgba.shape[:2]
    g = guides(pto, scene, w, h)
    return g, filter(rgba, g, p)
