"""ctypes binding of tests/census_ref/libcensus_ref.so — the scalar walker of docs/SPEC.md §5 that counts the branch class of every
path vertex (tests/material_zoo.py names the classes). Test infrastructure only, like oracle/pto.py; `build()` runs its Makefile."""
import ctypes as C
import os
import subprocess

import numpy as np

from material_zoo import CLASSES

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "census_ref")
_lib = None


class cr_stats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("paths", C.c_uint64), ("n", C.c_uint64 * (len(CLASSES) + 1))]


def build():
    """make the walker (incremental) and load it."""
    global _lib
    subprocess.run(["make", "-s", "-C", DIR], check=True)
    if _lib is None:
        _lib = C.CDLL(os.path.join(DIR, "libcensus_ref.so"))
        _lib.cr_render.restype = C.c_int
        _lib.cr_render.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(cr_stats)]
        assert _lib.cr_num_classes() == len(CLASSES) + 1
    return _lib


def render(pto, scene, params, threads=0):
    """(rgba float32 HxWx4, rays, paths, {class: count}, inconsistent) of one frame. `scene`: a pto.Scene; `params`: any ctypes
    struct with the pt_render_params layout. `inconsistent` counts vertices whose restated branch condition contradicts the
    sampler's own outputs; it must be 0."""
    lib = build()
    p = pto.pto_params()
    C.memmove(C.byref(p), C.byref(params), C.sizeof(pto.pto_params))
    out = np.zeros((p.height, p.width, 4), np.float32)
    st = cr_stats()
    rc = lib.cr_render(C.addressof(scene.c), C.addressof(p), threads, out.ctypes.data, C.byref(st))
    if rc != 0:
        raise RuntimeError(f"cr_render failed: {rc}")
    return out, int(st.rays), int(st.paths), {c: int(st.n[i]) for i, c in enumerate(CLASSES)}, int(st.n[len(CLASSES)])
