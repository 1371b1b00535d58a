"""The lens space, stated once for tests/test_lens_space.py (no device) and tests/test_gpu_lens_space.py: named lenses on both sides of
the thresholds of docs/SPEC.md §3.1 "Domain", the cross of lenses and cameras (tests/camera_space.py has the cameras), the scenes, the
RNG draws of a frame's camera rays, and the judgement of a frame of primitive ids against the float64 caster (tests/ray_caster64.py) on
the float64 rays of tests/lens64.py. Test helpers only.

Pytest rewrites `assert` only in test modules, so every assert here carries its own message."""
import ctypes as C
import dataclasses
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import adversarial_scenes as S
import camera_space as cs
import lens64 as L
import ray_caster64 as rc
from float64_support import ALLOWED

W, H = cs.W, cs.H
SEED = 0x5EED0001  # make_params' default
SAMPLES = 4        # the id frames: sample_offset = 0 .. 3, one sample each

# name -> (R, F), every value exact in f32
LENS_CASES = {
    "moderate": (float(np.float32(0.05)), 2.5),            # the three lenses of test_gpu_lens.LENSES
    "almost_pinhole": (float(np.float32(1e-3)), 1e3),
    "wide_open": (0.5, 0.25),
    "near_pinhole": (2.0 ** -20, 1.0),
    "absorbed": (2.0 ** -20, 2.0 ** 20),                   # fma(F, v, -a) returns F v
    "far_focus": (float(np.float32(0.05)), 2.0 ** 30),
    "tiny": (2.0 ** -30, 2.0 ** -30),
    "huge_aperture": (2.0 ** 20, 1.0),
    "focus_2p63": (float(np.float32(0.05)), 2.0 ** 63),    # the last F before dot(w, w) overflows under a camera of unit length ...
    "focus_2p64": (float(np.float32(0.05)), 2.0 ** 64),    # ... and the first after it
    "aperture_2p63": (2.0 ** 63, 1.0),
    "aperture_2p64": (2.0 ** 64, 1.0),
    "both_2m70": (2.0 ** -70, 2.0 ** -70),                 # dot(w, w) is a subnormal: a direction right to four digits
    "both_1em30": (float(np.float32(1e-30)), float(np.float32(1e-30))),  # dot(w, w) underflows to 0: an infinite direction
}
MODERATE = "moderate"
# under the `default` camera: the lens that must be refused -> its neighbour on the other side of the threshold, which must be right
OUT_OF_DOMAIN = {"focus_2p64": "focus_2p63", "aperture_2p64": "aperture_2p63", "both_2m70": "tiny", "both_1em30": "tiny"}
ALL_LENS_CAMERAS = ("default", "skewed", "anisotropic", "far", "long_forward")
SCALED = "scaled_2p40"       # `default` with forward, right and up times 2^40: far_focus, in the domain under `default`, leaves it
REFUSED_CAMERAS = ("flat_basis",)  # right and up span no plane: no lens is accepted (a zero right or up: test_gpu_lens.py)
SCENES = ("triangle", "spheres", "box")


def cross():
    """[(lens name, camera name)]: every lens under five cameras, the moderate lens under every camera §3.1 accepts, and far_focus
    under the scaled basis."""
    out = [(lens, cam) for lens in LENS_CASES for cam in ALL_LENS_CAMERAS]
    out += [(MODERATE, cam) for cam in cs.CASE_NAMES if cam not in ALL_LENS_CAMERAS and cam not in REFUSED_CAMERAS]
    return out + [("far_focus", SCALED)]


SPHERE_REACH = 64.0     # SPEC §4: a sphere's silhouette is uncertain by 1 % of r^2 at 147 radii, 66 units for the radius 0.45 of `spheres`
BOX_REACH = 256.0       # `box` has triangles 0.1 units wide; an f32 ray from L units away is uncertain by about 5 * 2^-24 L there, and the
#                         samples that close to an edge pass 1 % near L = 1000 (measured under `far`: 1.8 to 2.2 %; 72 % from 2^20)
LENGTH_REACH = 2.0 ** 30  # SPEC §4: coordinates within 2^±30
REACH = {"triangle": LENGTH_REACH, "spheres": SPHERE_REACH, "box": BOX_REACH}


def scenes_of(P, lens, cam):
    """The scenes whose hits are judged under (lens name, camera name): those inside the domain SPEC §4 states for the closest hit, by
    the reach of a ray's origin — the camera's distance from the scene's middle plus the aperture's radius. `spheres` up to SPHERE_REACH
    and `box` up to BOX_REACH (not from `far`'s 1000 units or through an aperture of 2^20), `triangle` up to LENGTH_REACH (not with an
    aperture of 2^63, which has no scene: its rays are held to float64 by the ray comparison alone)."""
    out = []
    for name in SCENES:
        sd = table(P, name)[cam]
        lo, hi = cs._bounds64(sd)
        reach = np.linalg.norm(cs.Cam64(sd.cam).o - 0.5 * (lo + hi)) + LENS_CASES[lens][0]
        if reach <= REACH[name]:
            out.append(name)
    return tuple(out)


_scenes, _tables = {}, {}


def scene(P, name):
    """(scene data under the generator camera, layout): cs.scene's triangle and spheres, and the tessellated Cornell box at 1000
    triangles asked for (1002 made, and the box's own spheres) under cs.SKY."""
    if name not in _scenes:
        if name == "box":
            _scenes[name] = (dataclasses.replace(P.make_scene(P.native.PT_SCENE_CORNELL_TESS, 1000, 5, W, H), sky=cs.SKY), 68)
        else:
            _scenes[name] = cs.scene(P, name, W, H)
    return _scenes[name]


def table(P, name):
    """{camera name: scene data} of scene `name`: cs.cases, and SCALED."""
    if name not in _tables:
        sd, _ = scene(P, name)
        t = dict(cs.cases(P, sd, W, H))
        c = cs.Cam64(t["default"].cam)
        c.f, c.r, c.u = c.f * 2.0 ** 40, c.r * 2.0 ** 40, c.u * 2.0 ** 40
        t[SCALED] = dataclasses.replace(t["default"], cam=c.stored(sd.cam))
        _tables[name] = t
    return _tables[name]


def with_jitter(sd, jitter):
    cam = type(sd.cam).from_buffer_copy(sd.cam)
    cam.jitter = jitter
    return dataclasses.replace(sd, cam=cam)


# ------------------------------------------------------------------------------------------------ the draws of a frame's camera rays
_draws = {}


def keys(pto, pixels, sample, seed=SEED):
    """The oracle's path keys of the (x, y) pixels of a W-wide frame at sample index `sample`."""
    return [pto.lib.pto_path_key(seed, y * W + x, sample) for x, y in pixels]


def draws_of(pto, key_list, jitter):
    """(n, 4) float32: (jx, jy, u2, u3) = u01(key, 0 .. 3) as the oracle's RNG gives them; jx = jy = 0.5 with the jitter off."""
    out = np.full((len(key_list), 4), 0.5, np.float32)
    for i, k in enumerate(key_list):
        for dim in range(0 if jitter else 2, 4):
            out[i, dim] = pto.lib.pto_u01(k, dim)
    return out


def frame_draws(pto):
    """(x, y, draws) of the SAMPLES id frames, sample-major: index s * W * H + y * W + x. The jitter is off (S.id_scene)."""
    if "frame" not in _draws:
        pixels = [(x, y) for y in range(H) for x in range(W)]
        x = np.tile(np.array([p[0] for p in pixels], np.float64), SAMPLES)
        y = np.tile(np.array([p[1] for p in pixels], np.float64), SAMPLES)
        _draws["frame"] = (x, y, np.concatenate([draws_of(pto, keys(pto, pixels, s), 0) for s in range(SAMPLES)]))
    return _draws["frame"]


# ------------------------------------------------------------------------------------------------ id frames against the caster
class Reference:
    """The float64 side of one (lens, camera, scene): lens64's rays of every (pixel, sample) of the id frames, their bounds, and the
    caster's closest hit on them. Made from the reference alone."""

    def __init__(self, pto, sd, lens):
        self.sd = S.id_scene(sd)
        self.lens = lens
        x, y, dr = frame_draws(pto)
        self.o, self.d = L.ray64(self.sd.cam, lens, x, y, dr)
        self.E_o, self.angle = L.ray_bound(self.sd.cam, lens, x, y, dr)
        self.cast = rc.cast(self.sd.verts, self.sd.spheres, self.o, self.d, rays64=True)

    def corners_disagree(self, idx):
        """For the rays idx: whether the caster's ids at the eight corners of ray_bound (each sign of the three components of E_o, the
        direction tilted by the angle along both axes across it, the signs taken in turn) differ among themselves or from the centre's."""
        o, d, want = self.o[idx], self.d[idx], self.cast[0][idx]
        helper = np.where(np.abs(d[:, :1]) < 0.9, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
        e1 = np.cross(d, helper)
        e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
        e2 = np.cross(d, e1)
        out = np.zeros(len(idx), bool)
        for j in range(8):
            sg = np.array([1.0 if j >> k & 1 else -1.0 for k in range(3)])
            dd = d + self.angle[idx, None] * (sg[0] * e1 + sg[1] * e2)
            ids = rc.cast(self.sd.verts, self.sd.spheres, o + sg * self.E_o[idx], dd / np.linalg.norm(dd, axis=1, keepdims=True), rays64=True)[0]
            out |= ids != want
        return out


def judge(ref, got):
    """The ids `got` (sample-major, MISS for none) of an f32 implementation against ref. A sample whose id differs from the caster's is
    undecidable if the reference alone says so — the caster's ids at the corners of ray_bound disagree, or rc.classify puts it in `edge`
    or `coincident` (the sphere band of SPEC §4 included) — and wrong otherwise. Returns (wrong indices, undecidable indices, samples)."""
    sd = ref.sd
    c = rc.classify(sd.verts, sd.spheres, ref.o, ref.d, got, ref.cast, sphere_band=True, rays64=True)
    excused = np.union1d(c["edge"], c["coincident"])
    differ = np.union1d(excused, c["wrong"])
    unstable = differ[ref.corners_disagree(differ)] if len(differ) else differ
    undecidable = np.union1d(excused, unstable)
    return np.setdiff1d(c["wrong"], unstable), undecidable, len(got)


def check(ref, got, ctx):
    """wrong == 0, the undecidable share within ALLOWED; returns that share."""
    wrong, undecidable, n = judge(ref, got)
    want = ref.cast[0]
    assert len(wrong) == 0, (ctx, len(wrong), wrong[:8].tolist(), np.asarray(got)[wrong[:8]].tolist(), want[wrong[:8]].tolist())
    assert len(undecidable) <= ALLOWED * n, (ctx, len(undecidable), n)
    return len(undecidable) / n


def frame_ids(render, P):
    """The ids of the SAMPLES id frames, sample-major. render(params) -> an H x W x 4 frame of the id scene."""
    out = []
    for s in range(SAMPLES):
        p = S.params_id(W, H)
        p.sample_offset = s
        out.append(S.ids_of(render(p)))
    return np.concatenate(out)


_refs = {}


def references(P, pto, triples):
    """{(lens name, camera name, scene name): Reference} for `triples`, made once per process, several at a time: the caster is numpy."""
    todo = [t for t in dict.fromkeys(triples) if t not in _refs]
    if todo:
        frame_draws(pto)
        for name in SCENES:
            table(P, name)
        workers = max(1, min(16, int(os.environ.get("OMP_NUM_THREADS", "8")), len(todo)))
        with ThreadPoolExecutor(workers) as pool:
            made = pool.map(lambda t: Reference(pto, table(P, t[2])[t[1]], LENS_CASES[t[0]]), todo)
            _refs.update(zip(todo, made))
    return {t: _refs[t] for t in triples}


def cam_copy(cam):
    c = type(cam)()
    C.memmove(C.byref(c), C.byref(cam), C.sizeof(c))
    return c
