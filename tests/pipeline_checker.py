"""ctypes binding of tests/pipeline_ref/ (pathtracing_amd/csrc/pipeline.h behind plain C): the library's own decode of a frame's
pipeline, callable without a device."""
import ctypes as C

import ref_lib


class Decoded(C.Structure):
    _fields_ = [("status", C.c_int32), ("message", C.c_char_p), ("forced", C.c_uint32),
                ("profile", C.c_uint32), ("count", C.c_uint32), ("split", C.c_uint32), ("bucket", C.c_uint32), ("nee", C.c_uint32),
                ("env", C.c_uint32), ("shade", C.c_int32), ("fuse", C.c_int32),
                ("full_state", C.c_uint32), ("resolves_sky", C.c_uint32), ("instrumented", C.c_uint32),
                ("single_loop", C.c_uint32 * 2), ("generate_mode", C.c_uint32 * 2), ("kernel_for", (C.c_int32 * 3) * 4)]


def build():
    return ref_lib.load("pipeline_ref", "libpipeline_ref.so", {
        "pr_decode": (None, [C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.POINTER(Decoded)]),
        "pr_forces_compact": (C.c_int, [C.c_uint32, C.c_int, C.c_uint32]),
        "pr_extend_instantiated": (C.c_int, [C.c_int] * 5),
        "pr_extend_kernel_first": (C.c_uint32, []),
        "pr_extend_kernel_last": (C.c_uint32, []),
    })


def decode(flags, tuned_kernel=0, env=False, specular=False):
    """The header's decode of (flags, pt_tuning.extend_kernel, environment present, specular materials present)."""
    d = Decoded()
    build().pr_decode(flags, tuned_kernel, int(env), int(specular), C.byref(d))
    return d
