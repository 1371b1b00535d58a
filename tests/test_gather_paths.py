"""CPU checks of pt_gather_paths (include/ptrt.h, docs/SPEC.md §12.1): they hold the scalar checker of tests/gather_paths_ref/, which the
device is compared with bit for bit (tests/test_gpu_gather_paths.py), to a known answer, to gather_ref at depth 1 and to the oracle's
path tracer; and the refusals that need no device, through the C ABI."""
import copy
import ctypes as C
import dataclasses

import numpy as np
import pytest

import gather_paths_checker as GP
import gather_ref as G
import nee_checker as nc

SKY = np.array([1.0, 2.0, 3.0], np.float32)
Z = 4.0  # the statistical test's bound, in standard deviations of the difference (the rule of tests/test_nee.py and tests/test_env.py)


def test_furnace_known_answer(P, pto):
    """A closed box whose every surface is Lambert with albedo 0.5 and emission 1, black sky, no roulette, D = 8 segments: a sample that
    ran all D segments brings 1 + 1/2 + ... + 2^(1-D) = 2 - 2^(1-D) exactly (every term a power of two), and a point all of whose 64 samples
    did has E exactly that: 64 equal terms, one per lane, a butterfly of exact doublings, one division by 64.
    The points are the first hits of the 24 x 18 frame of the box before its front is walled up — they lie inside the closed box (the
    frame of the closed box itself sees only the outside of the new wall, from where every path leaves into the void). A sample that ends
    early can only have slipped through an edge; at most 1 % of the points may be excluded for that (measured: none, 0 of 306)."""
    D, K = 8, 64
    sd = GP.furnace_scene(P, G)
    pts, nrm = G.first_hits(P, pto, P.make_scene(P.native.PT_SCENE_CORNELL, 0, 3, G.W, G.H))
    assert len(pts) >= 257
    r = GP.gather(pto.Scene(sd), pts, nrm, samples=K, max_depth=D, rr_start=D, per_sample=True)
    full = r.sample_segs == D
    whole = full.all(1)
    print(f"furnace: {(~full).sum()} of {full.size} samples ended early, {(~whole).sum()} of {len(pts)} points excluded")
    assert (~whole).sum() <= 0.01 * len(pts)
    want = np.float32(2.0 - 2.0 ** (1 - D))
    assert (r.sample_rad[full] == want).all()
    assert (r.E[whole] == want).all()
    assert r.rays == int(r.sample_segs.sum()) and (r.visibility[whole] == 0).all() and (r.bent[whole] == 0).all()


@pytest.mark.parametrize("name", ["glass", "tess"])
def test_depth_one_is_the_sky_gather(P, pto, name):
    """max_depth = 1 on a scene without emitters is §12: E within gather_ref's (K + 2) 2^-24 bound, the counts exactly and bent within
    the bound, unbounded and with max_distance about half the box; one segment per sample."""
    sd, pts, nrm, rays = G.case(P, pto, name)
    dark = dataclasses.replace(GP.without_emission(sd), sky=SKY)
    osc = pto.Scene(dark)
    b = (G.K + 2) * 2.0 ** -24
    for md in (0.0, G.half_box(sd)):
        ref = G.gather(rays, md, sky=SKY)
        r = GP.gather(osc, pts, nrm, samples=G.K, max_distance=md, ray_eps=G.EPS, max_depth=1, rr_start=0)
        assert r.rays == G.K * len(pts)
        assert np.array_equal(np.rint(r.visibility.astype(np.float64) * G.K).astype(np.int64), ref["count"]), md
        assert (np.abs(r.bent.astype(np.float64) - ref["bent"]) <= b).all(), md
        if md == 0.0:  # (with a finite max_distance §12's E also takes the sky behind an occluder farther than that; a path does not)
            assert (np.abs(r.E.astype(np.float64) - ref["E"]) <= b * ref["absE"]).all()
    assert 0 < ref["count"].sum() < G.K * len(pts)


def _white_pixels(P, pto, sd, osc, w, h):
    """(x, y, point, normal, albedo) of the pixels whose centre ray first hits a white, non-emissive Lambert triangle."""
    v = np.asarray(sd.verts, np.float32).reshape(-1, 3, 3)
    pc = pto.pto_camera()
    C.memmove(C.byref(pc), C.byref(sd.cam), C.sizeof(pto.pto_camera))
    o, d = (C.c_float * 3)(), (C.c_float * 3)()
    out = []
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
            out.append((x, y, (oo.astype(np.float64) + t * dd.astype(np.float64)).astype(np.float32), (n / np.linalg.norm(n)).astype(np.float32), float(a[0])))
    return out


@pytest.mark.parametrize("kind", ["PT_SCENE_CORNELL", "PT_SCENE_CORNELL_GLASS"])
def test_agrees_with_the_oracles_path_tracer(P, pto, kind):
    """A pixel of pto_render whose (unjittered) camera ray first hits a white Lambert surface that does not emit estimates albedo * E at
    that point: the camera path's first vertex multiplies by the albedo and continues like a gathered sample (one depth further on, so
    the frame runs max_depth + 1 and rr_start + 1). Eight such pixels of an 8 x 6 frame of C1 and C4, 65536 samples each way (the
    gather in 16 sample ranges): per pixel and channel the two means agree within 4 sigma of their combined standard error, and each of
    the checker's three deliberate errors fails the same check. Measured largest distances, C1 / C4: correct 1.8 / 1.7 sigma; first
    emission dropped 40.8 / 42.2; throughput without W 40.8 / 38.3; survivors not divided by qrr 11.1 / 11.2 (at 4096 samples the last
    stood at 3.7 to 3.9 sigma, so the counts were enlarged, not the rule loosened)."""
    W, H, SPP, KG, CALLS, D, R = 8, 6, 65536, 4096, 16, 8, 1
    sd = P.make_scene(getattr(P.native, kind), 0, 3, W, H)
    cam = copy.deepcopy(sd.cam)
    cam.jitter = 0
    sd = dataclasses.replace(sd, cam=cam)
    osc = pto.Scene(sd)
    osc.build_own_bvh()
    params = P.make_params(W, H, spp=SPP, max_depth=D + 1, rr_start=R + 1, streams=1, seed=11)
    img, st, sq = nc.render(pto, osc, params, flags=0, with_sq=True)
    ref, ost = pto.render(osc, params)
    assert np.array_equal(img, ref) and st.ext_rays == ost.rays  # the moments are those of the oracle's own frame
    m = img[..., :3].astype(np.float64)
    var = (sq / SPP - m * m) * SPP / (SPP - 1)
    white = _white_pixels(P, pto, sd, osc, W, H)
    sel = white[::max(1, len(white) // 8)][:8]
    assert len(sel) == 8
    pts, nrm = np.array([s[2] for s in sel]), np.array([s[3] for s in sel])

    def max_z(flags):
        rad = np.concatenate([GP.gather(osc, pts, nrm, samples=KG, seed=5, sample_offset=c * KG, max_depth=D, rr_start=R, ray_eps=params.ray_eps,
                                        flags=flags, per_sample=True).sample_rad.astype(np.float64) for c in range(CALLS)], axis=1)
        mg, vg = rad.mean(1), rad.var(1, ddof=1)
        return max(float((np.abs(m[y, x] - a * mg[i]) / np.sqrt(var[y, x] / SPP + a * a * vg[i] / (KG * CALLS))).max())
                   for i, (x, y, _, _, a) in enumerate(sel))

    z = {f: max_z(f) for f in (0, GP.NO_FIRST_EMISSION, GP.NO_W, GP.NO_RR_DIV)}
    print(kind, {k: round(v, 2) for k, v in z.items()})
    assert z[0] < Z, z
    for f in (GP.NO_FIRST_EMISSION, GP.NO_W, GP.NO_RR_DIV):
        assert z[f] > Z, (f, z)


def test_exported_with_the_documented_argtypes(P):
    N = P.native
    assert hasattr(N.lib, "pt_gather_paths")
    res, args = N.SYMBOLS["pt_gather_paths"]
    assert res is C.c_int32
    assert args == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(N.pt_gather_params), C.POINTER(N.pt_gather_path_params),
                    C.POINTER(N.pt_stats)]
    assert C.sizeof(N.pt_gather_path_params) == 32
    assert [f[0] for f in N.pt_gather_path_params._fields_] == ["max_depth", "rr_start", "flags", "pad"]
    assert N.lib.pt_abi_version() == 2 and hasattr(P.Renderer, "GatherPaths")


def test_refused_without_a_device(P):
    """pp's checks come first (NULL, a flag bit, max_depth 256), then every check of pt_gather in its order: a bad path block is reported
    even when gp is bad or missing too, and a good one lets gp's refusals through with the call's own name in the message."""
    N = P.native
    pts = np.zeros((4, 8), np.float32)
    pts[:, 5] = 1.0
    out = np.zeros((4, 8), np.float32)
    st = N.pt_stats()
    host = N.PT_GATHER_HOST_MEMORY

    def call(ctx, scene, gp, pp, points=pts, rows=out):
        return N.lib.pt_gather_paths(ctx, scene, None if points is None else points.ctypes.data_as(C.c_void_p),
                                     None if rows is None else rows.ctypes.data_as(C.c_void_p), 4, None if gp is None else C.byref(gp),
                                     None if pp is None else C.byref(pp), C.byref(st))

    err = lambda: N.lib.pt_last_error(None)
    PP = N.pt_gather_path_params
    bad_gp = N.pt_gather_params(flags=2, samples=5000, max_distance=-1.0, ray_eps=-1.0)
    for gp in (None, bad_gp, N.pt_gather_params(flags=host)):
        assert call(None, None, gp, None) == N.PT_ERR_INVALID_ARGUMENT and b"path params is NULL" in err()
        for bit in (1, 2, 0x80000000):
            assert call(None, None, gp, PP(flags=bit)) == N.PT_ERR_INVALID_ARGUMENT and b"unknown path flag" in err()
        assert call(None, None, gp, PP(max_depth=256)) == N.PT_ERR_INVALID_ARGUMENT and b"255" in err()
        assert call(None, None, gp, PP(max_depth=256, flags=1)) == N.PT_ERR_INVALID_ARGUMENT and b"unknown path flag" in err()
    for good in (PP(), PP(max_depth=255, rr_start=0xFFFFFFFF), PP(max_depth=1)):  # now gp's checks, in pt_gather's order
        assert call(None, None, None, good) == N.PT_ERR_INVALID_ARGUMENT and b"pt_gather_paths: params is NULL" in err()
        assert call(None, None, bad_gp, good) == N.PT_ERR_INVALID_ARGUMENT and b"unknown flag" in err()
        assert call(None, None, N.pt_gather_params(samples=5000, max_distance=-1.0, ray_eps=-1.0), good) == N.PT_ERR_INVALID_ARGUMENT and b"4096" in err()
        assert call(None, None, N.pt_gather_params(max_distance=-1.0, ray_eps=-1.0), good) == N.PT_ERR_INVALID_ARGUMENT and b"max_distance" in err()
        assert call(None, None, N.pt_gather_params(ray_eps=float("nan")), good) == N.PT_ERR_INVALID_ARGUMENT and b"ray_eps" in err()
        ok = N.pt_gather_params(samples=4096, flags=host)
        assert call(None, None, ok, good) == N.PT_ERR_INVALID_ARGUMENT and b"pt_gather_paths: NULL argument" in err()
        s = C.c_void_p()
        assert N.lib.pt_scene_create(None, C.byref(s)) == N.PT_OK
        try:
            assert call(None, s, ok, good) == N.PT_ERR_INVALID_ARGUMENT and b"NULL argument" in err()
            assert call(None, s, ok, good, points=None) == N.PT_ERR_INVALID_ARGUMENT and call(None, s, ok, good, rows=None) == N.PT_ERR_INVALID_ARGUMENT
        finally:
            N.lib.pt_scene_destroy(s)
    assert (out == 0).all()
