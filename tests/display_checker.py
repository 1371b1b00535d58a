"""ctypes binding of tests/display_ref/libdisplay_ref.so — the scalar restatement of docs/SPEC.md §10 (pt_display) that the display
tests check the device against. Test infrastructure only, like tests/temporal_checker.py; `build()` runs its Makefile.

The adaptation state is explicit: `display()` takes the previous exposure (or None) and returns the next one. The threshold table comes
from tests/golden/srgb8_thresholds.json, not from the product."""
import ctypes as C
import json
import os

import numpy as np

import ref_lib

HERE = os.path.dirname(os.path.abspath(__file__))
AUTO, LINEAR, RESET = 1, 2, 4
CLAMP, REINHARD, ACES = 0, 1, 2
FRAME, DENOISED, TEMPORAL = 0, 1, 2
# dr_display variants: §10 as written, then the deliberately wrong ones of the negative controls
SPEC, QUANTISE_FIRST, ARITHMETIC_MEAN, NO_TRIM = range(4)
_table = None


class dr_params(C.Structure):
    _fields_ = [("source", C.c_uint32), ("curve", C.c_uint32), ("exposure", C.c_float), ("white", C.c_float), ("key", C.c_float),
                ("adapt", C.c_float), ("trim_low", C.c_uint32), ("trim_high", C.c_uint32), ("flags", C.c_uint32), ("pad", C.c_uint32)]


class dr_info(C.Structure):
    _fields_ = [("exposure", C.c_float), ("metered", C.c_float), ("log_average", C.c_float), ("adapted", C.c_uint32),
                ("counted", C.c_uint64), ("used", C.c_uint64)]


assert C.sizeof(dr_params) == 40 and C.sizeof(dr_info) == 32


# name -> (restype, argtypes): the entry points of display_ref.c
SYMBOLS = {
    "dr_resolve": (C.c_int, [C.POINTER(dr_params), C.POINTER(dr_params)]),
    "dr_luminance": (C.c_float, [C.c_float, C.c_float, C.c_float]),
    "dr_bin": (C.c_int, [C.c_float]),
    "dr_unorm8": (C.c_uint8, [C.c_float]),
    "dr_srgb8": (C.c_uint8, [C.c_void_p, C.c_float]),
    "dr_display": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(dr_params), C.c_int, C.c_void_p, C.c_int, C.c_float,
                             C.c_void_p, C.c_void_p, C.POINTER(dr_info), C.POINTER(C.c_int), C.POINTER(C.c_float)]),
}


def build():
    """The checker, made (incrementally) and loaded on the first call of a process."""
    return ref_lib.load("display_ref", "libdisplay_ref.so", SYMBOLS)


def table():
    """T as 256 float32 (T[0] = 0, never compared), from the committed bit patterns."""
    global _table
    if _table is None:
        bits = json.load(open(os.path.join(HERE, "golden", "srgb8_thresholds.json")))["bits"]
        assert len(bits) == 255
        _table = np.concatenate([np.zeros(1, np.uint32), np.array(bits, np.uint32)]).view(np.float32)
    return _table


def params(source=FRAME, curve=CLAMP, exposure=0.0, white=0.0, key=0.0, adapt=0.0, trim_low=0, trim_high=0, flags=0):
    return dr_params(source, curve, exposure, white, key, adapt, trim_low, trim_high, flags)


def resolve(p):
    """The parameters with §10's defaults filled in, or None where §10 refuses them."""
    out = dr_params()
    return out if build().dr_resolve(C.byref(p), C.byref(out)) == 0 else None


def bin_of(y):
    """§10's bin of one luminance (float32 bits kept), or -1 for a pixel that is not counted."""
    return build().dr_bin(C.c_float(np.float32(y)))


def srgb8(y):
    """The sRGB8 codes of an array of float32 values in [0, 1]."""
    lib, t = build(), table()
    return np.array([lib.dr_srgb8(t.ctypes.data, C.c_float(v)) for v in np.asarray(y, np.float32).ravel()], np.uint8).reshape(np.shape(y))


class Result:
    def __init__(self, image, histogram, info, state):
        self.image, self.histogram, self.info, self.state = image, histogram, info, state


def info_tuple(info):
    """A pt_display_info / dr_info as comparable bits: the three floats as u32, then the integers."""
    f = np.array([info.exposure, info.metered, info.log_average], np.float32).view(np.uint32)
    return (int(f[0]), int(f[1]), int(f[2]), int(info.adapted), int(info.counted), int(info.used))


def display(image, p=None, state=None, variant=SPEC):
    """§10 for one call: (h, w, 4) float32 source, its parameters and the adaptation state before the call (None, or the last adapted
    exposure as a float32). Returns a Result: (h, w, 4) uint8 image, the 512 bins, the dr_info and the state after the call."""
    image = np.ascontiguousarray(image, np.float32)
    h, w = image.shape[:2]
    assert image.shape == (h, w, 4)
    out = np.zeros((h, w, 4), np.uint8)
    hist = np.zeros(512, np.uint32)
    info, have_next, nxt = dr_info(), C.c_int(0), C.c_float(0.0)
    t = table()
    rc = build().dr_display(image.ctypes.data, h * w, C.byref(p if p is not None else params()), variant, t.ctypes.data,
                            0 if state is None else 1, C.c_float(0.0 if state is None else np.float32(state)),
                            out.ctypes.data, hist.ctypes.data, C.byref(info), C.byref(have_next), C.byref(nxt))
    if rc != 0:
        raise ValueError("dr_display refused the parameters")
    return Result(out, hist, info, np.float32(nxt.value) if have_next.value else None)
