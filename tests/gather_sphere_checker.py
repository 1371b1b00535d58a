"""ctypes binding of tests/gather_sphere_ref/libgather_sphere_ref.so — the scalar restatement of docs/SPEC.md §12.2 with §7.1's sphere lights
(pt_gather_paths with PT_GATHER_PATHS_NEXT_EVENT | PT_GATHER_PATHS_SPHERE_LIGHTS) that the device is held to bit for bit, `rays` included.
Test infrastructure only, like oracle/pto.py; the first call runs its Makefile (ref_lib)."""
import ctypes as C
import dataclasses

import numpy as np

import ref_lib

NO_MIS, NO_POINT_SAMPLE, NO_COSL, NO_PSEL, POINT_TW_ALBEDO = 1, 2, 4, 8, 16  # tests/gather_nee_ref's deliberate errors
SPHERES = 32                                                                 # PT_GATHER_PATHS_SPHERE_LIGHTS
HITS_WEIGHT_1, AREA_PDF, SWAP_PMF = 64, 128, 256                             # the deliberate errors of the sphere lights' controls


class gsr_params(C.Structure):
    _fields_ = [("samples", C.c_uint32), ("seed", C.c_uint32), ("sample_offset", C.c_uint32), ("point_offset", C.c_uint32),
                ("max_distance", C.c_float), ("ray_eps", C.c_float), ("max_depth", C.c_uint32), ("rr_start", C.c_uint32)]


class gsr_stats(C.Structure):
    _fields_ = [("segments", C.c_uint64), ("shadow_rays", C.c_uint64), ("n_lights", C.c_uint64), ("n_sphere_lights", C.c_uint64),
                ("lit", C.c_uint32), ("pad", C.c_uint32)]


SYMBOLS = {
    "gsr_gather": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(gsr_params), C.c_uint32, C.c_int, C.c_void_p, C.c_uint64,
                             C.c_void_p, C.POINTER(gsr_stats), C.c_void_p]),
}


def build():
    return ref_lib.load("gather_sphere_ref", "libgather_sphere_ref.so", SYMBOLS)


@dataclasses.dataclass
class Result:
    rows: np.ndarray          # (n, 8) f32 output records
    segments: int             # path segments traced: the unflagged call's rays
    shadow_rays: int          # shadow rays traced
    n_lights: int             # §7's NL (triangles)
    n_sphere_lights: int      # §7.1's sphere lights (0 without SPHERES)
    lit: bool                 # §11: the map is a light
    sample_rad: np.ndarray    # (n, K, 3) f32 per-sample radiance, or None

    @property
    def rays(self):
        return self.segments + self.shadow_rays

    @property
    def E(self):
        return self.rows[:, 0:3]


def gather(scene, points, normals, samples=64, seed=0, sample_offset=0, point_offset=0, max_distance=0.0, ray_eps=1e-3, max_depth=8,
           rr_start=3, env=None, flags=SPHERES, per_sample=False, threads=0):
    """§12.2 + §7.1 on the CPU. `scene`: a pto.Scene; env: (n, n, 3) texels or None. samples and max_depth 0 mean their defaults (64, 8)."""
    lib = build()
    samples, max_depth = samples or 64, max_depth or 8
    rec = np.zeros((len(points), 8), np.float32)
    rec[:, 0:3], rec[:, 4:7] = np.asarray(points, np.float32).reshape(-1, 3), np.asarray(normals, np.float32).reshape(-1, 3)
    rows = np.zeros_like(rec)
    p = gsr_params(samples, seed & 0xFFFFFFFF, sample_offset & 0xFFFFFFFF, point_offset & 0xFFFFFFFF, max_distance, ray_eps, max_depth, rr_start)
    e = None if env is None else np.ascontiguousarray(env, np.float32)
    rad = np.zeros((len(rec), samples, 3), np.float32) if per_sample else None
    st = gsr_stats()
    rc = lib.gsr_gather(C.addressof(scene.c), None if e is None else e.ctypes.data, 0 if e is None else e.shape[0], C.byref(p), flags, threads,
                        rec.ctypes.data, len(rec), rows.ctypes.data, C.byref(st), None if rad is None else rad.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"gsr_gather failed: {rc}")
    return Result(rows, int(st.segments), int(st.shadow_rays), int(st.n_lights), int(st.n_sphere_lights), bool(st.lit), rad)


def call(P, r, rec, samples=64, host=True, next_event=True, sphere_lights=True, max_depth=8, rr_start=3, **kw):
    """pt_gather_paths through the C ABI with PT_GATHER_PATHS_NEXT_EVENT | PT_GATHER_PATHS_SPHERE_LIGHTS (or without either) on the (n, 8)
    records: (out (n, 8) float32, pt_stats). host=False: through device tensors. Four rows behind `out` must keep their bytes."""
    N = P.native
    n = len(rec)
    gp = N.pt_gather_params(samples=samples, seed=kw.get("seed", 0), sample_offset=kw.get("sample_offset", 0),
                            point_offset=kw.get("point_offset", 0), max_distance=kw.get("max_distance", 0.0),
                            ray_eps=kw.get("ray_eps", 1e-3), flags=N.PT_GATHER_HOST_MEMORY if host else 0)
    flags = (N.PT_GATHER_PATHS_NEXT_EVENT if next_event else 0) | (N.PT_GATHER_PATHS_SPHERE_LIGHTS if sphere_lights else 0)
    pp = N.pt_gather_path_params(max_depth=max_depth, rr_start=rr_start, flags=flags)
    st = N.pt_stats()
    rec = np.ascontiguousarray(rec, np.float32)
    if host:
        out = np.full((n + 4, 8), 7.0, np.float32)
        a, b = rec.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    else:
        import torch
        d_rec = torch.as_tensor(rec, device="cuda")
        d_out = torch.full((n + 4, 8), 7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        a, b = C.c_void_p(d_rec.data_ptr()), C.c_void_p(d_out.data_ptr())
    rc = N.lib.pt_gather_paths(r._ctx, r._scene, a, b, n, C.byref(gp), C.byref(pp), C.byref(st))
    assert rc == N.PT_OK, (rc, N.lib.pt_last_error(r._ctx))
    if not host:
        out = d_out.cpu().numpy()
    assert (out[n:] == 7.0).all(), ("guard band", n, samples, out[n:])
    return out[:n], st
