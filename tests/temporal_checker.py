"""ctypes binding of tests/temporal_ref/libtemporal_ref.so — the scalar restatement of docs/SPEC.md §9 (pt_denoise_temporal) that the
temporal tests check the device against. Test infrastructure only, like tests/denoise_checker.py; `build()` runs its Makefile.

The history is explicit: `accumulate()` takes a `History` (or None) and returns the next one."""
import ctypes as C

import numpy as np

import ref_lib

RESET, MATCH_IDS = 1, 2
MISS = 0xFFFFFFFF
# tr_accumulate variants: §9 as written, then the deliberately wrong ones of the negative controls
SPEC, NO_REPROJECTION, NO_PLANE_TEST, NEAREST_TAP, FIXED_ALPHA = range(5)


class tr_params(C.Structure):
    _fields_ = [("max_history", C.c_uint32), ("plane_tolerance", C.c_float), ("normal_min", C.c_float), ("flags", C.c_uint32),
                ("pad", C.c_uint32 * 4)]


class tr_camera(C.Structure):  # pt_camera / pto_camera
    _fields_ = [("origin", C.c_float * 3), ("forward", C.c_float * 3), ("right", C.c_float * 3), ("up", C.c_float * 3),
                ("scale", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("jitter", C.c_uint32)]


assert C.sizeof(tr_params) == 32 and C.sizeof(tr_camera) == 64


# name -> (restype, argtypes): the entry points of temporal_ref.c
SYMBOLS = {
    "tr_resolve": (C.c_int, [C.POINTER(tr_params), C.POINTER(tr_params)]),
    "tr_accumulate": (C.c_long, [C.c_void_p, C.c_void_p, C.POINTER(tr_camera), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                 C.POINTER(tr_camera), C.POINTER(tr_params), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
}


def build():
    """The checker, made (incrementally) and loaded on the first call of a process."""
    return ref_lib.load("temporal_ref", "libtemporal_ref.so", SYMBOLS)


def params(max_history=0, plane_tolerance=0.0, normal_min=0.0, flags=0):
    return tr_params(max_history, plane_tolerance, normal_min, flags)


def defaults():
    """The §9 defaults the checker restates (max_history, tau_p, tau_n)."""
    out = tr_params()
    assert build().tr_resolve(C.byref(params()), C.byref(out)) == 0
    return out.max_history, out.plane_tolerance, out.normal_min


def camera(cam):
    """A copy of any ctypes struct with the pt_camera layout."""
    c = tr_camera()
    C.memmove(C.byref(c), C.byref(cam), C.sizeof(tr_camera))
    return c


class History:
    """What a successful call leaves for the next: its guides, accumulated rgb | length, and camera."""

    def __init__(self, g8, h, cam):
        self.g8, self.h, self.cam = g8, h, cam

    @property
    def shape(self):
        return self.h.shape[:2]


class Result:
    def __init__(self, image, length, history, taken, reproj):
        self.image, self.length, self.history, self.taken, self.reproj = image, length, history, taken, reproj


def accumulate(frame, g8, cam, history=None, p=None, variant=SPEC, want_reproj=False):
    """§9 for one call: (h, w, 4) float32 frame, (h, w, 8) guides of this call, its camera and the previous call's History (None, or one
    of another size: no history). Returns a Result: accumulated image (h, w, 4), lengths (h, w), the new History, the number of pixels
    that took history and, with want_reproj, (h, w, 3) = (fx, fy, valid)."""
    frame = np.ascontiguousarray(frame, np.float32)
    g8 = np.ascontiguousarray(g8, np.float32)
    h, w = frame.shape[:2]
    assert frame.shape == (h, w, 4) and g8.shape == (h, w, 8)
    if history is not None and history.shape != (h, w):
        history = None  # a size change restarts the history
    cam = camera(cam)
    out, new_h = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
    reproj = np.zeros((h, w, 3), np.float32) if want_reproj else None
    n = build().tr_accumulate(frame.ctypes.data, g8.ctypes.data, C.byref(cam), w, h,
                              history.g8.ctypes.data if history is not None else None,
                              history.h.ctypes.data if history is not None else None,
                              C.byref(history.cam) if history is not None else None,
                              C.byref(p if p is not None else params()), variant, out.ctypes.data, new_h.ctypes.data,
                              reproj.ctypes.data if want_reproj else None)
    if n < 0:
        raise ValueError("tr_accumulate refused the parameters")
    return Result(out, new_h[..., 3].copy(), History(g8, new_h, cam), int(n), reproj)
