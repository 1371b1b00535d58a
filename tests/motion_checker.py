"""ctypes binding of tests/motion_ref/libmotion_ref.so — the scalar restatement of docs/SPEC.md §9 with §9.1 (pt_denoise_temporal with
PT_TEMPORAL_MOTION) that the motion tests check the device against. Test infrastructure only, like tests/temporal_checker.py; `build()`
runs its Makefile.

The history and the snapshot are explicit: `accumulate()` takes a `History` (or None) and returns the next one. A History carries the
snapshot its call recorded (flagged calls only) and a `scene_key` of the caller's choosing: §9.1's "same scene object, no commit since" is
`history.scene_key == scene_key`."""
import ctypes as C

import numpy as np

import ref_lib

RESET, MATCH_IDS, MOTION = 1, 2, 8
MISS = 0xFFFFFFFF
# mr_accumulate variants: the spec as written, then the deliberately wrong ones of the negative controls
SPEC, IGNORE_MOTION, NEW_PLANE, NEW_NORMAL, NO_RADIUS_RATIO = range(5)


class mr_params(C.Structure):
    _fields_ = [("max_history", C.c_uint32), ("plane_tolerance", C.c_float), ("normal_min", C.c_float), ("flags", C.c_uint32),
                ("pad", C.c_uint32 * 4)]


class mr_camera(C.Structure):  # pt_camera / pto_camera
    _fields_ = [("origin", C.c_float * 3), ("forward", C.c_float * 3), ("right", C.c_float * 3), ("up", C.c_float * 3),
                ("scale", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("jitter", C.c_uint32)]


assert C.sizeof(mr_params) == 32 and C.sizeof(mr_camera) == 64


# name -> (restype, argtypes): the entry points of motion_ref.c
SYMBOLS = {
    "mr_resolve": (C.c_int, [C.POINTER(mr_params), C.POINTER(mr_params)]),
    "mr_accumulate": (C.c_long, [C.c_void_p, C.c_void_p, C.POINTER(mr_camera), C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32,
                                 C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(mr_camera), C.c_void_p, C.c_void_p,
                                 C.POINTER(mr_params), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_long)]),
}


def build():
    """The checker, made (incrementally) and loaded on the first call of a process."""
    return ref_lib.load("motion_ref", "libmotion_ref.so", SYMBOLS)


def params(max_history=0, plane_tolerance=0.0, normal_min=0.0, flags=0):
    return mr_params(max_history, plane_tolerance, normal_min, flags)


def camera(cam):
    """A copy of any ctypes struct with the pt_camera layout."""
    c = mr_camera()
    C.memmove(C.byref(c), C.byref(cam), C.sizeof(mr_camera))
    return c


class History:
    """What a successful call leaves for the next: its guides, accumulated rgb | length and camera; after a flagged call also the
    triangles (NT, 9) and spheres (NS, 4) it was traced on and the caller's key of the scene they were recorded from."""

    def __init__(self, g8, h, cam, snap_tris=None, snap_sph=None, scene_key=None):
        self.g8, self.h, self.cam, self.snap_tris, self.snap_sph, self.scene_key = g8, h, cam, snap_tris, snap_sph, scene_key

    @property
    def shape(self):
        return self.h.shape[:2]

    @property
    def has_snapshot(self):
        return self.snap_tris is not None


class Result:
    def __init__(self, image, length, history, taken, moved, moved_mask, reproj, used_snapshot):
        self.image, self.length, self.history, self.taken, self.moved = image, length, history, taken, moved
        self.moved_mask, self.reproj, self.used_snapshot = moved_mask, reproj, used_snapshot


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def accumulate(frame, g8, cam, verts, spheres, history=None, p=None, variant=SPEC, want_reproj=False, scene_key=0):
    """§9 + §9.1 for one call: (h, w, 4) float32 frame, (h, w, 8) guides of this call, its camera, the scene's current triangles (NT, 9)
    and spheres (NS, 4), and the previous call's History (None, or one of another size: no history). The snapshot of `history` is used
    when `p` has MOTION, the history counts and `history.scene_key == scene_key` with the same primitive counts. Returns a Result:
    accumulated image (h, w, 4), lengths (h, w), the new History (with a snapshot iff `p` has MOTION), the number of pixels that took
    history, the number of hit pixels whose primitive counted as moved with their (h, w) mask and, with want_reproj, (h, w, 3) = (fx, fy,
    valid)."""
    frame = np.ascontiguousarray(frame, np.float32)
    g8 = np.ascontiguousarray(g8, np.float32)
    verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 9)
    spheres = np.ascontiguousarray(spheres, np.float32).reshape(-1, 4)
    h, w = frame.shape[:2]
    assert frame.shape == (h, w, 4) and g8.shape == (h, w, 8)
    if history is not None and history.shape != (h, w):
        history = None  # a size change restarts the history
    p = p if p is not None else params()
    cam = camera(cam)
    snap_t = snap_s = None
    if (history is not None and history.has_snapshot and history.scene_key == scene_key and history.snap_tris.shape == verts.shape
            and history.snap_sph.shape == spheres.shape):
        snap_t, snap_s = history.snap_tris, history.snap_sph
    out, new_h = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
    reproj = np.zeros((h, w, 3), np.float32) if want_reproj else None
    mask = np.zeros((h, w), np.uint8)
    n_moved = C.c_long(0)
    n = build().mr_accumulate(frame.ctypes.data, g8.ctypes.data, C.byref(cam), w, h, _ptr(verts), len(verts), _ptr(spheres), len(spheres),
                              history.g8.ctypes.data if history is not None else None,
                              history.h.ctypes.data if history is not None else None,
                              C.byref(history.cam) if history is not None else None,
                              _ptr(snap_t), _ptr(snap_s), C.byref(p), variant, out.ctypes.data, new_h.ctypes.data,
                              reproj.ctypes.data if want_reproj else None, mask.ctypes.data, C.byref(n_moved))
    if n < 0:
        raise ValueError("mr_accumulate refused the parameters")
    flagged = bool(p.flags & MOTION)
    used = flagged and snap_t is not None and not (p.flags & RESET) and p.max_history != 1
    nxt = History(g8, new_h, cam, verts.copy() if flagged else None, spheres.copy() if flagged else None, scene_key if flagged else None)
    return Result(out, new_h[..., 3].copy(), nxt, int(n), int(n_moved.value), mask.astype(bool), reproj, used)
