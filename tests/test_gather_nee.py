"""CPU checks of PT_GATHER_PATHS_NEXT_EVENT (include/ptrt.h, docs/SPEC.md §12.2): the flag's plumbing and its refusals without a device,
and the scalar checker of tests/gather_nee_ref/ — which the device is compared with bit for bit (tests/test_gpu_gather_nee.py) — held
to the unflagged checker of tests/gather_paths_ref/: the same call where there is no light, the same segments, visibility and bent
everywhere, the same expectation, a lower variance, and finite records at grazing and point-blank lights."""
import copy
import ctypes as C
import dataclasses
import inspect
import os
import re

import numpy as np
import pytest

import env_checker
import gather_nee_checker as GN
import gather_paths_checker as GP
import gather_ref as G
import nee_checker as nc
from gather_device import SKY, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = 4.0  # the statistical test's bound, in standard deviations of the difference (the rule of tests/test_nee.py and tests/test_env.py)
W, H, KG, CALLS, R = 8, 6, 4096, 16, 1  # the frame whose pixels give the points; 65536 samples in 16 sample ranges; rr_start
ASSERTED_RATIO = 38.0  # half of the measured variance ratio of test 6
MIN_EVENTS = 64  # a point takes part if at least this many of the plain checker's samples bring anything (see _points)


def test_the_flag(P):
    """1. PT_GATHER_PATHS_NEXT_EVENT = 4u in the header, the Python binding and the C# binding; Renderer.GatherPaths takes next_event;
    without a device pp.flags = 4 passes pp's checks and reaches gp's, while every other bit is still refused first."""
    N = P.native
    hdr = open(os.path.join(ROOT, "include", "ptrt.h")).read()
    assert re.search(r"PT_GATHER_PATHS_NEXT_EVENT\s*=\s*4u", hdr)
    assert N.PT_GATHER_PATHS_NEXT_EVENT == 4
    cs = open(os.path.join(ROOT, "host", "csharp", "PtrtNative.cs")).read()
    assert re.search(r"enum PtGatherPathFlags : uint \{ NextEvent = 4 \}", cs)
    assert "nextEvent" in open(os.path.join(ROOT, "host", "csharp", "HipRenderer.cs")).read()
    assert inspect.signature(P.Renderer.GatherPaths).parameters["next_event"].default is False
    assert C.sizeof(N.pt_gather_path_params) == 32 and N.lib.pt_abi_version() == 2
    pts, out, st = np.zeros((4, 8), np.float32), np.zeros((4, 8), np.float32), N.pt_stats()

    def call(gp, pp):
        return N.lib.pt_gather_paths(None, None, pts.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), 4, None if gp is None else C.byref(gp),
                                     C.byref(pp), C.byref(st))

    err = lambda: N.lib.pt_last_error(None)
    PP = N.pt_gather_path_params
    assert call(None, PP(flags=4)) == N.PT_ERR_INVALID_ARGUMENT and b"pt_gather_paths: params is NULL" in err() and b"unknown path flag" not in err()
    assert call(N.pt_gather_params(flags=N.PT_GATHER_HOST_MEMORY), PP(flags=4, max_depth=1)) == N.PT_ERR_INVALID_ARGUMENT and b"NULL argument" in err()
    assert call(None, PP(flags=4, max_depth=256)) == N.PT_ERR_INVALID_ARGUMENT and b"255" in err()
    for bits in (4 | 1, 4 | 2, 8, 4 | 0x80000000):
        assert call(None, PP(flags=bits)) == N.PT_ERR_INVALID_ARGUMENT and b"unknown path flag" in err(), bits
    assert (out == 0).all()


def _glass(P, pto):
    sd = G.scene(P, "glass")
    pts, nrm = G.first_hits(P, pto, sd)
    return sd, pts, nrm


def test_no_light_is_the_unflagged_call(P, pto):
    """2. Without an emissive triangle and without a map, and under an all-black map, the flagged checker is the unflagged checker bit for
    bit, rows and rays: no shadow ray, no weight."""
    sd, pts, nrm = _glass(P, pto)
    dark = dataclasses.replace(GP.without_emission(sd), sky=SKY)
    osc = pto.Scene(dark)
    for env in (None, np.zeros((8, 8, 3), np.float32)):
        for md in (8, 1):
            a = GN.gather(osc, pts, nrm, env=env, max_depth=md, ray_eps=G.EPS)
            b = GP.gather(osc, pts, nrm, env=env, max_depth=md, ray_eps=G.EPS)
            assert a.n_lights == 0 and not a.lit and a.shadow_rays == 0
            assert same(a.rows, b.rows) and a.rays == b.rays


@pytest.mark.parametrize("name", ["glass", "lights", "grazing"])
def test_same_segments_visibility_and_bent(P, pto, name):
    """3. §12.2 draws dimensions of its own: the BSDF-sampled paths are the unflagged call's. The segments are its rays, and visibility
    and bent its bits, for an unbounded and a bounded max_distance."""
    sd = {"glass": lambda: G.scene(P, "glass"), "lights": lambda: nc.many_lights_scene(P, G.W, G.H), "grazing": lambda: nc.grazing_scene(P, G.W, G.H)}[name]()
    pts, nrm = G.first_hits(P, pto, sd)
    osc = pto.Scene(sd)
    for dist in (0.0, G.half_box(sd)):
        a = GN.gather(osc, pts, nrm, max_distance=dist, ray_eps=G.EPS)
        b = GP.gather(osc, pts, nrm, max_distance=dist, ray_eps=G.EPS)
        assert a.n_lights > 0 and a.shadow_rays > 0 and a.segments == b.rays
        assert same(a.rows[:, 3:], b.rows[:, 3:]) and not same(a.rows[:, :3], b.rows[:, :3])


# ------------------------------------------------------------------------------------------------ the statistical tests
def _white_points(pto, sd, osc, w, h):
    """(points, normals) where the centre rays of a w x h frame first hit a white, non-emissive Lambert triangle."""
    v = np.asarray(sd.verts, np.float32).reshape(-1, 3, 3)
    pc = pto.pto_camera()
    C.memmove(C.byref(pc), C.byref(sd.cam), C.sizeof(pto.pto_camera))
    o, d = (C.c_float * 3)(), (C.c_float * 3)()
    pts, nrm = [], []
    for y in range(h):
        for x in range(w):
            pto.lib.pto_camera_ray(C.byref(pc), x, y, 0, o, d)
            oo, dd = np.array(o[:], np.float32), np.array(d[:], np.float32)
            pid, t = osc.closest(oo, dd)
            if pid >= len(v):
                continue
            m = sd.mats[sd.tri_mat[pid]]
            a = m["albedo"]
            if m["kind"] != 0 or m["emission"].any() or not (a[0] == a[1] == a[2]):
                continue
            n = np.cross(v[pid, 1] - v[pid, 0], v[pid, 2] - v[pid, 0]).astype(np.float64)
            n = -n if (n * dd).sum() > 0 else n
            pts.append((oo.astype(np.float64) + t * dd.astype(np.float64)).astype(np.float32))
            nrm.append((n / np.linalg.norm(n)).astype(np.float32))
    return np.array(pts), np.array(nrm)


def _unjittered(sd):
    cam = copy.deepcopy(sd.cam)
    cam.jitter = 0
    return dataclasses.replace(sd, cam=cam)


def _moments(fn, osc, pts, nrm, env, md, **kw):
    rad = np.concatenate([fn(osc, pts, nrm, samples=KG, seed=5, sample_offset=c * KG, max_depth=md, rr_start=R, env=env, per_sample=True,
                             **kw).sample_rad.astype(np.float64) for c in range(CALLS)], axis=1)
    return rad.mean(1), rad.var(1, ddof=1), (rad != 0).any(2).sum(1)


def _points(P, pto, name, md):
    """(osc, env, points, normals, the plain checker's moments there): eight points on white, non-emissive Lambert surfaces. C1 and C4: where
    the unjittered centre rays of an 8 x 6 frame first hit such a surface; the soup, which that frame hardly hits, is white Lambert
    throughout: centroids of its triangles. A point takes part only if at least MIN_EVENTS of the plain checker's 65536 samples bring
    anything: a mean over fewer events is not near normal and its sample variance says nothing (a ceiling point at max_depth 1 sees the
    ceiling light at a cosine of 1e-3; the plain estimator finds it about once in 10^7 samples, its mean and variance are 0 exactly and
    every difference is then infinitely many 'sigma'). The rule looks at the unflagged reference only."""
    kind, env = {"C1": ("cornell", None), "C4": ("glass", None), "C1+sun": ("cornell", env_checker.sun_sky(P)),
                 "soup+sun": ("soup", env_checker.sun_sky(P))}[name]
    sd = _unjittered(env_checker.scene(P, kind, W, H))
    osc = pto.Scene(sd)
    osc.build_own_bvh()
    if kind == "soup":
        pts, nrm = G.centroids(sd, every=7)
    else:
        pts, nrm = _white_points(pto, sd, osc, W, H)
    mp, vp, events = _moments(GP.gather, osc, pts, nrm, env, md)
    ok = np.nonzero(events >= MIN_EVENTS)[0]
    sel = ok[::max(1, len(ok) // 8)][:8]
    assert len(sel) == 8, (name, md, len(ok))
    return osc, env, pts[sel], nrm[sel], mp[sel], vp[sel]


_Z = {}


def _max_z(P, pto, name, md):
    """Per deliberate error (0: none), the largest distance between the flagged and the plain mean over the eight points and three
    channels, in standard errors of the difference. Computed once per (scene, depth)."""
    if (name, md) not in _Z:
        osc, env, pts, nrm, mp, vp = _points(P, pto, name, md)
        z = {}
        for f in (0, *GN.ERRORS.values()):
            mn, vn, _ = _moments(GN.gather, osc, pts, nrm, env, md, flags=f)
            z[f] = float((np.abs(mp - mn) / np.sqrt((vp + vn) / (KG * CALLS))).max())
        print(name, md, {k: round(v, 2) for k, v in z.items()})
        _Z[(name, md)] = z
    return _Z[(name, md)]


SCENES = ["C1", "C4", "C1+sun", "soup+sun"]


@pytest.mark.parametrize("md", [8, 1])
@pytest.mark.parametrize("name", SCENES)
def test_unbiased(P, pto, name, md):
    """4. Eight points on white non-emissive Lambert surfaces, 65536 samples in 16 sample ranges each way: the flagged and the plain
    checker's means agree per point and channel within 4 sigma of their combined standard error, on C1 (a triangle light), C4 (specular
    vertices: rays with pb = 0), C1 under the sun map (both kinds, psel = 0.5) and the soup under the sun map (the map only); with
    max_depth 8 and with max_depth 1, the direct-light bake. Measured largest distances, max_depth 8 / 1: C1 2.2 / 1.7, C4 1.8 / 1.7,
    C1 + sun 2.5 / 1.6, soup + sun 1.4 / 1.5 sigma."""
    z = _max_z(P, pto, name, md)
    assert z[0] < Z, z


@pytest.mark.parametrize("flag", sorted(GN.ERRORS))
def test_negative_controls(P, pto, flag):
    """5. Each of the checker's deliberate errors exceeds the bound of test 4 on at least one of its scenes. Measured largest |z| per
    flag over the scenes and both depths: NO_MIS 95.8 (soup + sun; C1 39.0), NO_POINT_SAMPLE 94.9 (C1 43.1), NO_COSL 251.2 (C1, depth 1;
    1.4 on the soup, which has no triangle light), NO_PSEL 48.1 (C1 + sun, the only scene with both kinds; elsewhere psel is 1 and the
    flag changes nothing), POINT_TW_ALBEDO 95.2 (C1 29.4)."""
    worst = max(_max_z(P, pto, name, md)[GN.ERRORS[flag]] for name in SCENES for md in (8, 1))
    print(flag, round(worst, 1))
    assert worst > Z, (flag, worst)


def test_variance_is_lower(P, pto):
    """6. On C1 at K = 64, over the first hits of the 24 x 18 frame, the per-sample variance of E (summed over the channels, averaged over
    the points) is lower with the flag. Measured with the two checkers: 76.2 x (the light is a small quad that a cosine-weighted
    direction rarely finds); half of it, 38, is asserted."""
    sd = env_checker.scene(P, "cornell", G.W, G.H)
    pts, nrm = G.first_hits(P, pto, sd)
    osc = pto.Scene(sd)
    var = lambda r: r.sample_rad.astype(np.float64).var(1, ddof=1).sum(1).mean()
    plain = var(GP.gather(osc, pts, nrm, samples=64, ray_eps=G.EPS, per_sample=True))
    nee = var(GN.gather(osc, pts, nrm, samples=64, ray_eps=G.EPS, per_sample=True))
    print("variance ratio", plain / nee)
    assert plain / nee >= ASSERTED_RATIO, plain / nee


def test_finite_at_grazing_and_point_blank_lights(P, pto):
    """7. grazing_scene with ray_eps 1e-4 and 0, and points on the emissive triangles themselves facing both ways: every output is
    finite, whatever the pdfs' quotients do."""
    sd = nc.grazing_scene(P, G.W, G.H)
    osc = pto.Scene(sd)
    pts, nrm = G.first_hits(P, pto, sd)
    v = np.asarray(sd.verts, np.float32).reshape(-1, 3, 3)
    lit = sd.mats["emission"].any(1)[sd.tri_mat]
    on = v[lit]
    lp = np.concatenate([on.mean(1), on[:, 0], 0.5 * (on[:, 0] + on[:, 1])])  # centroids, corners and edge midpoints of the lights
    ln = np.cross(on[:, 1] - on[:, 0], on[:, 2] - on[:, 0])
    ln = np.tile(ln / np.linalg.norm(ln, axis=1, keepdims=True), (3, 1)).astype(np.float32)
    lp, ln = G.both_sides(lp, ln)
    for eps in (1e-4, 0.0):
        for p_, n_ in ((pts, nrm), (lp, ln)):
            for md in (8, 1):
                r = GN.gather(osc, p_, n_, ray_eps=eps, max_depth=md, per_sample=True)
                assert np.isfinite(r.rows).all() and np.isfinite(r.sample_rad).all() and r.shadow_rays > 0


def test_product_does_not_reference_the_checker():
    """8. The product neither includes, links nor names the checker."""
    for top in ("pathtracing_amd", "include", "host"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith((".py", ".cpp", ".h", ".hpp", ".hip", ".cs", "Makefile")):
                    txt = open(os.path.join(dirpath, f), errors="replace").read()
                    assert "gather_nee_ref" not in txt and "gather_nee_checker" not in txt and "gnr_gather" not in txt, f
