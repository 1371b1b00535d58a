"""ctypes binding of tests/gather_paths_ref/libgather_paths_ref.so — the scalar restatement of docs/SPEC.md §12.1 (pt_gather_paths) that
the device is held to bit for bit, `rays` included. Test infrastructure only, like oracle/pto.py; `build()` runs its Makefile."""
import ctypes as C
import dataclasses

import numpy as np

import ref_lib

NO_FIRST_EMISSION, NO_W, NO_RR_DIV = 1, 2, 4  # the deliberate errors of the negative controls


class gpr_params(C.Structure):
    _fields_ = [("samples", C.c_uint32), ("seed", C.c_uint32), ("sample_offset", C.c_uint32), ("point_offset", C.c_uint32),
                ("max_distance", C.c_float), ("ray_eps", C.c_float), ("max_depth", C.c_uint32), ("rr_start", C.c_uint32)]


SYMBOLS = {
    "gpr_gather": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(gpr_params), C.c_uint32, C.c_int, C.c_void_p, C.c_uint64,
                             C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p]),
}


def build():
    return ref_lib.load("gather_paths_ref", "libgather_paths_ref.so", SYMBOLS)


@dataclasses.dataclass
class Result:
    rows: np.ndarray          # (n, 8) f32 output records
    rays: int                 # segments traced, exact
    sample_rad: np.ndarray    # (n, K, 3) f32 per-sample radiance, or None
    sample_segs: np.ndarray   # (n, K) uint32 per-sample segment counts, or None

    @property
    def E(self):
        return self.rows[:, 0:3]

    @property
    def visibility(self):
        return self.rows[:, 3]

    @property
    def bent(self):
        return self.rows[:, 4:7]


def gather(scene, points, normals, samples=64, seed=0, sample_offset=0, point_offset=0, max_distance=0.0, ray_eps=1e-3, max_depth=8,
           rr_start=3, env=None, flags=0, per_sample=False, threads=0):
    """§12.1 on the CPU. `scene`: a pto.Scene (brute force or with a blob: the hits are the same); env: (n, n, 3) texels or None.
    samples and max_depth 0 mean their defaults (64, 8), as in the call."""
    lib = build()
    samples, max_depth = samples or 64, max_depth or 8
    rec = np.zeros((len(points), 8), np.float32)
    rec[:, 0:3], rec[:, 4:7] = np.asarray(points, np.float32).reshape(-1, 3), np.asarray(normals, np.float32).reshape(-1, 3)
    rows = np.zeros_like(rec)
    p = gpr_params(samples, seed & 0xFFFFFFFF, sample_offset & 0xFFFFFFFF, point_offset & 0xFFFFFFFF, max_distance, ray_eps, max_depth, rr_start)
    e = None if env is None else np.ascontiguousarray(env, np.float32)
    rad = np.zeros((len(rec), samples, 3), np.float32) if per_sample else None
    segs = np.zeros((len(rec), samples), np.uint32) if per_sample else None
    rays = C.c_uint64()
    rc = lib.gpr_gather(C.addressof(scene.c), None if e is None else e.ctypes.data, 0 if e is None else e.shape[0], C.byref(p), flags, threads,
                        rec.ctypes.data, len(rec), rows.ctypes.data, C.byref(rays), None if rad is None else rad.ctypes.data,
                        None if segs is None else segs.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"gpr_gather failed: {rc}")
    return Result(rows, int(rays.value), rad, segs)


def furnace_scene(P, G):
    """gather_ref's closed box with every material Lambert, albedo 0.5, emission 1, under a black sky."""
    sd = G.scene(P, "closed")
    mats = np.array(sd.mats, copy=True)
    for m in mats:
        m["kind"], m["albedo"], m["emission"], m["roughness"], m["ior"] = 0, (0.5, 0.5, 0.5), (1.0, 1.0, 1.0), 0.0, 1.0
    return dataclasses.replace(sd, mats=mats, sky=np.zeros(3, np.float32))


def without_emission(sd):
    mats = np.array(sd.mats, copy=True)
    mats["emission"] = 0.0
    return dataclasses.replace(sd, mats=mats)
