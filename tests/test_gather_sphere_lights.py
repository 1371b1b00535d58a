"""CPU checks of PT_GATHER_PATHS_SPHERE_LIGHTS (include/ptrt.h, docs/SPEC.md §7.1 in §12.2): the flag's plumbing and its refusals without a
device, and the scalar checker of tests/gather_sphere_ref/ — which the device is compared with bit for bit
(tests/test_gpu_gather_sphere_lights.py) — held to the checkers it extends: tests/gather_nee_ref/ where no sphere is a light and without
the flag, tests/gather_paths_ref/ for the segments, visibility, bent and the expectation; a lower variance, and finite records at
degenerate lamps."""
import ctypes as C
import dataclasses
import inspect
import os
import re

import numpy as np
import pytest

import gather_nee_checker as GN
import gather_paths_checker as GP
import gather_ref as G
import gather_sphere_checker as GS
import nee_checker as nc
import sphere_light_checker as sc
from gather_device import same
from test_gather_nee import _unjittered, _white_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = 4.0  # the statistical test's bound, in standard deviations of the difference (the rule of tests/test_nee.py)
W, H, KG, CALLS, R = 8, 6, 4096, 16, 1  # the frame whose pixels give the points; 65536 samples in 16 sample ranges; rr_start
MIN_EVENTS = 64  # a point takes part if at least this many of the plain checker's samples bring anything (tests/test_gather_nee.py)
MEASURED_VARIANCE_RATIO = 112.6  # test 6: unflagged NEE / flagged on the lamp-only Cornell
ASSERTED_RATIO = 0.5 * MEASURED_VARIANCE_RATIO


def test_the_flag(P):
    """1. PT_GATHER_PATHS_SPHERE_LIGHTS = 16u in the header, the Python binding and the C# binding; Renderer.GatherPaths takes
    sphere_lights; without a device 4 | 16 passes pp's checks and reaches gp's, 16 alone is refused by name, and bit 8 is still an
    unknown path flag."""
    N = P.native
    hdr = open(os.path.join(ROOT, "include", "ptrt.h")).read()
    assert re.search(r"PT_GATHER_PATHS_SPHERE_LIGHTS\s*=\s*16u", hdr)
    assert N.PT_GATHER_PATHS_SPHERE_LIGHTS == 16
    assert re.search(r"\bSphereLights\s*=\s*16\b", open(os.path.join(ROOT, "host", "csharp", "PtrtNative.cs")).read())
    assert "sphereLights" in open(os.path.join(ROOT, "host", "csharp", "HipRenderer.cs")).read()
    assert inspect.signature(P.Renderer.GatherPaths).parameters["sphere_lights"].default is False
    assert C.sizeof(N.pt_gather_path_params) == 32 and N.lib.pt_abi_version() == 2
    pts, out, st = np.zeros((4, 8), np.float32), np.zeros((4, 8), np.float32), N.pt_stats()

    def call(gp, pp):
        return N.lib.pt_gather_paths(None, None, pts.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), 4, None if gp is None else C.byref(gp),
                                     C.byref(pp), C.byref(st))

    err = lambda: N.lib.pt_last_error(None)
    PP = N.pt_gather_path_params
    assert call(None, PP(flags=4 | 16)) == N.PT_ERR_INVALID_ARGUMENT and b"pt_gather_paths: params is NULL" in err()
    assert call(None, PP(flags=16)) == N.PT_ERR_INVALID_ARGUMENT and b"PT_GATHER_PATHS_SPHERE_LIGHTS needs PT_GATHER_PATHS_NEXT_EVENT" in err()
    for bits in (8, 4 | 8, 4 | 16 | 8, 16 | 1, 4 | 16 | 32):
        assert call(None, PP(flags=bits)) == N.PT_ERR_INVALID_ARGUMENT and b"unknown path flag" in err(), bits
    assert (out == 0).all()


def _points(P, pto, sd):
    pts, nrm = G.first_hits(P, pto, sd)
    return pto.Scene(sd), pts, nrm


def test_no_sphere_light_is_the_nee_call(P, pto):
    """2. On scenes without a sphere light (C4, whose spheres do not emit, and the many-lights scene with its sphere's emission
    removed), with and without a map, the flagged checker is gather_nee_checker bit for bit, rows and rays."""
    for sd in (G.scene(P, "glass"), sc.without_sphere_emission(nc.many_lights_scene(P, G.W, G.H))):
        osc, pts, nrm = _points(P, pto, sd)
        for env in (None, sc.lit_map(P, 8)):
            for md in (8, 1):
                a = GS.gather(osc, pts, nrm, env=env, max_depth=md, ray_eps=G.EPS)
                b = GN.gather(osc, pts, nrm, env=env, max_depth=md, ray_eps=G.EPS)
                assert a.n_sphere_lights == 0 and a.n_lights == b.n_lights > 0 and a.shadow_rays > 0
                assert same(a.rows, b.rows) and (a.segments, a.shadow_rays) == (b.segments, b.shadow_rays)


@pytest.mark.parametrize("name", ["lamp", "lamp+quad", "glass-lamp", "lights"])
def test_unflagged_stays_and_the_paths_are_the_plain_ones(P, pto, name):
    """3. On scenes with sphere lights: without SPHERES the checker is gather_nee_checker bit for bit; with it the segments are the
    unflagged call's rays and visibility and bent its bits, for an unbounded and a bounded max_distance."""
    sd = nc.many_lights_scene(P, G.W, G.H) if name == "lights" else sc.scene(P, name, G.W, G.H)
    osc, pts, nrm = _points(P, pto, sd)
    for dist in (0.0, G.half_box(sd)):
        u = GS.gather(osc, pts, nrm, max_distance=dist, ray_eps=G.EPS, flags=0)
        n = GN.gather(osc, pts, nrm, max_distance=dist, ray_eps=G.EPS)
        assert same(u.rows, n.rows) and (u.segments, u.shadow_rays) == (n.segments, n.shadow_rays)
        a = GS.gather(osc, pts, nrm, max_distance=dist, ray_eps=G.EPS)
        b = GP.gather(osc, pts, nrm, max_distance=dist, ray_eps=G.EPS)
        assert a.n_sphere_lights >= 1 and a.shadow_rays > 0 and a.segments == b.rays
        assert same(a.rows[:, 3:], b.rows[:, 3:]) and not same(a.rows[:, :3], u.rows[:, :3])


# ------------------------------------------------------------------------------------------------ the statistical tests
CASES = {"lamp": ("lamp", False), "lamp+quad": ("lamp+quad", False), "lamp+quad+map": ("lamp+quad", True), "glass-lamp": ("glass-lamp", False),
         "two-lamps": ("two-lamps", False)}
ERRORS = {"HITS_WEIGHT_1": GS.HITS_WEIGHT_1, "AREA_PDF": GS.AREA_PDF, "SWAP_PMF": GS.SWAP_PMF, "NO_PSEL": GS.NO_PSEL}


def _moments(fn, osc, pts, nrm, env, md, **kw):
    rad = np.concatenate([fn(osc, pts, nrm, samples=KG, seed=5, sample_offset=c * KG, max_depth=md, rr_start=R, env=env, per_sample=True,
                             **kw).sample_rad.astype(np.float64) for c in range(CALLS)], axis=1)
    return rad.mean(1), rad.var(1, ddof=1), (rad != 0).any(2).sum(1)


_Z = {}


def _max_z(P, pto, name, md):
    """Per deliberate error (0: none), the largest distance between the flagged and the plain mean over eight points on white,
    non-emissive Lambert surfaces and three channels, in standard errors of the difference. The points are where the unjittered centre
    rays of an 8 x 6 frame first hit such a surface, thinned to eight; a point takes part only if at least MIN_EVENTS of the plain
    checker's 65536 samples bring anything (tests/test_gather_nee.py says why). Computed once per (scene, depth)."""
    if (name, md) not in _Z:
        scene, with_map = CASES[name]
        sd = _unjittered(sc.scene(P, scene, W, H))
        env = sc.lit_map(P) if with_map else None
        osc = pto.Scene(sd)
        osc.build_own_bvh()
        pts, nrm = _white_points(pto, sd, osc, W, H)
        mp, vp, events = _moments(GP.gather, osc, pts, nrm, env, md)
        ok = np.nonzero(events >= MIN_EVENTS)[0]
        sel = ok[::max(1, len(ok) // 8)][:8]
        assert len(sel) == 8, (name, md, len(ok))
        z = {}
        for f in (0, *ERRORS.values()):
            mn, vn, _ = _moments(GS.gather, osc, pts[sel], nrm[sel], env, md, flags=GS.SPHERES | f)
            z[f] = float((np.abs(mp[sel] - mn) / np.sqrt((vp[sel] + vn) / (KG * CALLS))).max())
        print(name, md, {k: round(v, 2) for k, v in z.items()})
        _Z[(name, md)] = z
    return _Z[(name, md)]


@pytest.mark.parametrize("md", [8, 1])
@pytest.mark.parametrize("name", list(CASES))
def test_unbiased(P, pto, name, md):
    """4. Eight points, 65536 samples in 16 sample ranges each way: the flagged and the plain checker's means agree per point and channel
    within 4 sigma of their combined standard error, with max_depth 8 and with max_depth 1 (the direct-light bake): lit by a lamp only,
    by the lamp and the quad, those under a lit map (psel = 1/2), by an emissive glass ball (weight-1 hits from inside), by two lamps.
    Measured largest distances, max_depth 8 / 1: 1.9 / 1.7, 2.5 / 1.3, 1.5 / 1.7, 1.3 / 1.6, 1.6 / 1.7 sigma."""
    z = _max_z(P, pto, name, md)
    assert z[0] < Z, z


@pytest.mark.parametrize("flag", sorted(ERRORS))
def test_negative_controls(P, pto, flag):
    """5. Each deliberate error misses the bound of test 4 by at least 3 Z on at least one of its scenes: sphere hits left at weight 1,
    the uniform-area pdf of the whole sphere, the pmfs of two lamps swapped, psel dropped. Measured largest |z| per error over the scenes and
    both depths: HITS_WEIGHT_1 34.0, AREA_PDF 108.6, SWAP_PMF 204.7 (the two-lamp scene; elsewhere the flag changes nothing), NO_PSEL 61.4
    (the scene under the map, the only one with psel = 1/2)."""
    worst = max(_max_z(P, pto, name, md)[ERRORS[flag]] for name in CASES for md in (8, 1))
    print(flag, round(worst, 1))
    assert worst > 3 * Z, (flag, worst)


def test_variance_is_lower(P, pto):
    """6. On the lamp-only Cornell at K = 64, over the first hits of the 24 x 18 frame, the per-sample variance of E (summed over the
    channels, averaged over the points) is lower with the flag than with PT_GATHER_PATHS_NEXT_EVENT alone, which finds the lamp by hits
    only. Half of the measured ratio (MEASURED_VARIANCE_RATIO) is asserted."""
    sd = sc.scene(P, "lamp", G.W, G.H)
    osc, pts, nrm = _points(P, pto, sd)
    var = lambda r: r.sample_rad.astype(np.float64).var(1, ddof=1).sum(1).mean()
    unflagged = var(GS.gather(osc, pts, nrm, samples=64, ray_eps=G.EPS, per_sample=True, flags=0))
    flagged = var(GS.gather(osc, pts, nrm, samples=64, ray_eps=G.EPS, per_sample=True))
    print("variance ratio", unflagged / flagged)
    assert unflagged / flagged >= ASSERTED_RATIO > 1.0, unflagged / flagged


def test_finite_at_degenerate_lamps(P, pto):
    """8. A lamp within ray_eps of the floor, one tangent to a wall, one the floor passes through, two overlapping lamps and a lamp of
    radius 2^-20; the frame's first hits and points on, inside and at the centre of the lamps, facing both ways, with ray_eps 1e-4
    and 0: every output is finite."""
    e, k = (6.0, 6.0, 6.0), (0.5, 0.5, 0.5)
    lamps = (((0.2, -1.0 + 0.1 + 5e-5, 0.3, 0.1), k, e, sc.LAMBERT), ((-1.0 + 0.2, 0.0, 0.0, 0.2), k, e, sc.LAMBERT),
             ((0.0, -1.0, -0.5, 0.4), k, e, sc.LAMBERT), ((0.5, 0.3, -0.4, 0.2), k, e, sc.LAMBERT), ((0.6, 0.35, -0.4, 0.2), k, e, sc.LAMBERT),
             ((-0.3, 0.5, 0.2, 2.0 ** -20), k, (1e9, 1e9, 1e9), sc.LAMBERT))
    sd = sc.cornell(P, G.W, G.H, lamps=lamps)
    osc, pts, nrm = _points(P, pto, sd)
    c, r = sd.spheres[-6:, :3], sd.spheres[-6:, 3:4]
    up = np.tile(np.array([[0.0, 1.0, 0.0]], np.float32), (6, 1))
    lp = np.concatenate([c + r * up, c + 0.5 * r * up, c])  # on the lamps, inside them, at their centres
    lp, ln = G.both_sides(lp.astype(np.float32), np.tile(up, (3, 1)))
    for eps in (1e-4, 0.0):
        for p_, n_ in ((pts, nrm), (lp, ln)):
            for md in (8, 1):
                res = GS.gather(osc, p_, n_, ray_eps=eps, max_depth=md, per_sample=True)
                assert res.n_sphere_lights == 6 and res.shadow_rays > 0
                assert np.isfinite(res.rows).all() and np.isfinite(res.sample_rad).all()


def test_product_does_not_reference_the_checker():
    for top in ("pathtracing_amd", "include", "host"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith((".py", ".cpp", ".h", ".hpp", ".hip", ".cs", "Makefile")):
                    txt = open(os.path.join(dirpath, f), errors="replace").read()
                    assert "gather_sphere_ref" not in txt and "gather_sphere_checker" not in txt and "gsr_gather" not in txt, f
