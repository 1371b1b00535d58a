"""ctypes binding of tests/census_ref/libcensus_ref.so — the scalar walker of docs/SPEC.md §5 that counts the branch class of every
path vertex (tests/material_zoo.py names the classes). Test infrastructure only, like oracle/pto.py; `build()` runs its Makefile."""
import ctypes as C

import numpy as np

from material_zoo import CLASSES

import ref_lib



class cr_stats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("paths", C.c_uint64), ("n", C.c_uint64 * (len(CLASSES) + 1))]


# name -> (restype, argtypes): the entry points of census_ref.c
SYMBOLS = {
    "cr_render": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(cr_stats)]),
    "cr_num_classes": (C.c_int, []),
}


def build():
    """The walker, made (incrementally) and loaded on the first call of a process."""
    lib = ref_lib.load("census_ref", "libcensus_ref.so", SYMBOLS)
    assert lib.cr_num_classes() == len(CLASSES) + 1
    return lib


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
