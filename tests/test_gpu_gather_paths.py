"""-m gpu: pt_gather_paths (include/ptrt.h, docs/SPEC.md §12.1) against the scalar checker of tests/gather_paths_ref/.

Every comparison is bit for bit — the eight floats of every record and pt_stats::rays. The points are the first hits of a 24 x 18 camera
frame (gather_ref.first_hits), K = 64 and ray_eps = 1e-3 unless a test says otherwise. Every test commits its own scene on the session's
renderer."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import env_checker
import gather_paths_checker as GP
import gather_ref as G
from gather_device import K, LBVH, SENTINEL, SKY, bits, call, other_state_is_untouched, same

pytestmark = pytest.mark.gpu


def held(P, r, osc, pts, nrm, ctx, env=None, host=True, **kw):
    """One call on the device and the checker's: the same bits, the same rays. Returns the device's (out, stats)."""
    out, st = call(P, r, G.records(pts, nrm), host=host, **kw)
    ref = GP.gather(osc, pts, nrm, env=env, **{"ray_eps": G.EPS, **kw})
    bad = np.nonzero((bits(out) != bits(ref.rows)).any(1))[0]
    assert len(bad) == 0, (ctx, len(bad), bad[:4], out[bad[:2]], ref.rows[bad[:2]])
    assert st.rays == ref.rays and st.paths == len(pts), (ctx, st.rays, ref.rays)
    assert np.isfinite(out).all()
    return out, st


def _case(P, pto, name, lit=None):
    sd = G.scene(P, name)
    pts, nrm = G.first_hits(P, pto, sd)
    osc = pto.Scene(sd)
    osc.build_own_bvh()
    return sd, pts, nrm, osc


@pytest.fixture(scope="module")
def glass(P, pto):
    return _case(P, pto, "glass")


@pytest.fixture(scope="module")
def tess(P, pto):
    return _case(P, pto, "tess")


def test_layouts(P, pto, renderer, glass, tess):
    """1. Cornell-glass (Lambert, metal, dielectric, spheres, the emissive quad) on BVH2 and the 2000-triangle Cornell under every
    layout and the GPU builder, with max_depth 8 / rr_start 3 and with max_depth 2: the checker's bits, and so the same on every layout."""
    sd, pts, nrm, osc = glass
    assert len(pts) >= 257 and len(sd.spheres) > 0 and {int(k) for k in sd.mats["kind"]} >= {0, 1, 2} and sd.mats["emission"].any()
    renderer.SetScene(sd, 2)
    for md, rr in ((8, 3), (2, 3)):
        out, st = held(P, renderer, osc, pts, nrm, ("glass", md), max_depth=md, rr_start=rr)
        assert (out[:, 0:3] > 0).any() and st.rays > K * len(pts) and st.gpu_ms > 0 and st.node_visits == 0 and st.iterations == 0
    sd, pts, nrm, osc = tess
    first = {}
    for width in (2, 4, 68, 72, 73, 68 | LBVH):
        renderer.SetScene(sd, width)
        for md, rr in ((8, 3), (2, 3)):
            out, _ = held(P, renderer, osc, pts, nrm, ("tess", width, md), max_depth=md, rr_start=rr)
            assert same(out, first.setdefault(md, out)), ("layouts differ", width, md)


@pytest.mark.parametrize("samples", [1, 5, 32, 100])
def test_group_shapes(P, pto, renderer, glass, samples):
    """2. K of 1, 5, 32 and 100 — several points per wave, lanes with g >= K, more than one sample per lane with regeneration in place
    — on 1 and 65 points (a last block partly beyond n) and on the whole set (more than one workgroup)."""
    sd, pts, nrm, osc = glass
    renderer.SetScene(sd, 0)
    for n in (1, 65, len(pts)):
        held(P, renderer, osc, pts[:n], nrm[:n], ("shape", n, samples), samples=samples)


def test_depth_and_roulette(P, pto, renderer, glass):
    """3. max_depth 1 and 255, rr_start 0 and beyond max_depth; and §12.1's consequences against pt_gather on the same renderer: (a)
    the visibility word and the bent row are pt_gather's bits for every max_distance, (b) with max_depth 1, max_distance 0 and no
    emitter the whole record is."""
    sd, pts, nrm, osc = glass
    renderer.SetScene(sd, 0)
    for md, rr in ((1, 0), (1, 3), (255, 0), (255, 255), (8, 8), (8, 0), (0, 3)):
        out, st = held(P, renderer, osc, pts, nrm, ("depth", md, rr), max_depth=md, rr_start=rr)
        assert md != 1 or st.rays == K * len(pts)
    rec = G.records(pts, nrm)
    for dist in (0.0, G.half_box(sd), 1e-4):
        sky, _ = call(P, renderer, rec, paths=False, max_distance=dist)
        for md in (1, 8):
            out, _ = call(P, renderer, rec, max_depth=md, max_distance=dist)
            assert same(out[:, 3:], sky[:, 3:]), ("(a)", dist, md)
    dark = dataclasses.replace(GP.without_emission(sd), sky=SKY)
    dosc = pto.Scene(dark)
    dosc.build_own_bvh()
    for scene, env in ((dark, None), (dataclasses.replace(dark, environment=env_checker.distinct(8)), env_checker.distinct(8))):
        renderer.SetScene(scene, 0)
        sky, _ = call(P, renderer, rec, paths=False)
        out, _ = held(P, renderer, dosc, pts, nrm, ("(b)", env is not None), env=env, max_depth=1, rr_start=0)
        assert same(out, sky) and (out[:, 0:3] > 0).any()


def test_environment_and_sky(P, pto, renderer, glass):
    """4. A map whose every texel has its own colour, and a constant sky, behind the open side of the box."""
    sd, pts, nrm, osc0 = glass
    lit = dataclasses.replace(sd, sky=SKY)
    osc = pto.Scene(lit)
    osc.build_own_bvh()
    renderer.SetScene(lit, 0)
    a, _ = held(P, renderer, osc, pts, nrm, "sky")
    env = env_checker.distinct(8)
    renderer.SetScene(dataclasses.replace(lit, environment=env), 0)
    b, _ = held(P, renderer, osc, pts, nrm, "map", env=env)
    c, _ = held(P, renderer, osc, pts, nrm, "map, half box", env=env, max_distance=G.half_box(sd))
    assert not same(a, b) and same(b[:, 0:3], c[:, 0:3]) and not same(b, c)  # the path does not see max_distance; visibility does


def test_merge_and_split(P, pto, renderer, glass):
    """5. (d): a bake split by point_offset is the unsplit bake, also where the cut falls inside a wave; the counts of the sample ranges
    [0, 32) and [32, 64) add up to that of [0, 64); a call repeats itself; another seed is another bake."""
    sd, pts, nrm, osc = glass
    rec = G.records(pts, nrm)
    renderer.SetScene(sd, 0)
    h = len(rec) // 2 + 1
    for samples in (K, 16):
        assert samples == K or h % 4 != 0
        one, s1 = call(P, renderer, rec, samples=samples)
        a, sa = call(P, renderer, rec[:h], samples=samples)
        b, sb = call(P, renderer, rec[h:], samples=samples, point_offset=h)
        assert same(np.concatenate([a, b]), one) and sa.rays + sb.rays == s1.rays
    whole, _ = call(P, renderer, rec)
    lo, sl = held(P, renderer, osc, pts, nrm, "lo", samples=32)
    hi, sh = held(P, renderer, osc, pts, nrm, "hi", samples=32, sample_offset=32)
    cnt = lambda o, k: np.rint(o[:, 3].astype(np.float64) * k).astype(np.int64)
    assert np.array_equal(cnt(lo, 32) + cnt(hi, 32), cnt(whole, K))
    again, _ = call(P, renderer, rec)
    other, _ = call(P, renderer, rec, seed=1)
    assert same(again, whole) and not same(other, whole)


def test_edge_inputs(P, pto, renderer, glass):
    """6. (c): invalid points among valid ones give the sentinel rows, trace nothing and leave their neighbours in the wave alone (4
    points per wave at K = 16); (e): sky values that overflow a lane's sum still give finite records, clamped to the largest float."""
    sd, pts, nrm, osc = glass
    renderer.SetScene(sd, 0)
    bad_p, bad_n = pts[:70].copy(), nrm[:70].copy()
    bad_p[5, 1] = np.nan
    bad_n[6, 0] = np.inf
    bad_n[41] = 0.0
    ok = np.ones(70, bool)
    ok[[5, 6, 41]] = False
    for samples in (16, K):
        clean, st0 = call(P, renderer, G.records(pts[:70], nrm[:70]), samples=samples)
        out, st = held(P, renderer, osc, bad_p, bad_n, ("invalid", samples), samples=samples)
        assert same(out[ok], clean[ok]) and (out[~ok] == SENTINEL).all() and st.rays < st0.rays
    hot = dataclasses.replace(sd, sky=np.array([3e38, 1e38, 3e37], np.float32))
    hosc = pto.Scene(hot)
    renderer.SetScene(hot, 0)
    out, _ = held(P, renderer, hosc, pts, nrm, "overflow")
    assert np.isfinite(out).all() and (out[:, 0] == np.float32(3.40282347e38)).any()


def test_interface_and_stats(P, pto, renderer, glass):
    """7. Host and device memory give the same bits; Renderer.GatherPaths takes numpy arrays and device tensors; the stats fields."""
    import torch
    sd, pts, nrm, osc = glass
    renderer.SetScene(sd, 0)
    out, st = held(P, renderer, osc, pts, nrm, "host")
    dev, sd_ = held(P, renderer, osc, pts, nrm, "device", host=False)
    assert same(dev, out) and sd_.rays == st.rays
    assert st.paths == len(pts) and st.gpu_ms > 0
    for f in ("node_visits", "tri_tests", "sphere_tests", "iterations"):
        assert getattr(st, f) == 0, f
    E, vis, bent, rst = renderer.GatherPaths(pts, nrm, samples=K, ray_eps=G.EPS, max_depth=8, rr_start=3)
    assert same(np.concatenate([E, vis[:, None], bent], 1), out[:, :7]) and rst.rays == st.rays
    tE, tvis, tbent, tst = renderer.GatherPaths(torch.as_tensor(pts, device="cuda"), torch.as_tensor(nrm, device="cuda"), samples=K, ray_eps=G.EPS,
                                                max_depth=8, rr_start=3)
    assert tE.is_cuda and same(tE.cpu().numpy(), E) and same(tvis.cpu().numpy(), vis) and same(tbent.cpu().numpy(), bent) and tst.rays == st.rays


def test_other_state_is_untouched(P, pto, glass):
    """7. A PT_FLAG_ACCUMULATE sequence with a pt_gather_paths in the middle is the sequence without it, and the denoised and displayed
    images, the guides and the temporal history of the frame survive the call."""
    sd, pts, nrm, _ = glass
    other_state_is_untouched(P, sd, G.records(pts, nrm), paths=True)


def test_refusals_that_need_a_context(P, pto, renderer, glass):
    """The checks behind the ones tests/test_gather_paths.py reaches without a device, in pt_gather's order and under this call's name;
    pp is still judged first; an empty batch is fine; max_depth 0 is 8."""
    N = P.native
    sd, pts, nrm, osc = glass
    renderer.SetScene(sd, 0)
    rec = np.zeros((5, 8), np.float32)
    rec[:, 5] = 1.0
    out = np.zeros((5, 8), np.float32)
    st = N.pt_stats()
    ctx = renderer._ctx
    err = lambda: N.lib.pt_last_error(ctx)

    def go(scene, p_off=0, o_off=0, n=4, flags=N.PT_GATHER_HOST_MEMORY, pp=None):
        gp = N.pt_gather_params(samples=4, flags=flags)
        pp = pp or N.pt_gather_path_params()
        return N.lib.pt_gather_paths(ctx, scene, C.c_void_p(rec.ctypes.data + p_off), C.c_void_p(out.ctypes.data + o_off), n, C.byref(gp),
                                     C.byref(pp), C.byref(st))

    fresh = C.c_void_p()
    assert N.lib.pt_scene_create(ctx, C.byref(fresh)) == N.PT_OK
    detached = C.c_void_p()
    assert N.lib.pt_scene_create(None, C.byref(detached)) == N.PT_OK
    try:
        assert go(fresh, p_off=2, pp=N.pt_gather_path_params(max_depth=256)) == N.PT_ERR_INVALID_ARGUMENT and b"255" in err()
        assert go(fresh, p_off=2) == N.PT_ERR_INVALID_ARGUMENT and b"pt_gather_paths: points and out must be 4-byte aligned" in err()
        assert go(fresh, o_off=4, flags=0) == N.PT_ERR_INVALID_ARGUMENT and b"16-byte aligned" in err()
        assert go(detached, n=1 << 32) == N.PT_ERR_INVALID_ARGUMENT and b"another context" in err()
        assert go(fresh, n=1 << 32) == N.PT_ERR_NOT_COMMITTED and b"not committed" in err()
        assert go(renderer._scene, n=1 << 32) == N.PT_ERR_INVALID_ARGUMENT and b"batch size" in err()
        assert go(renderer._scene, flags=0) == N.PT_ERR_INVALID_ARGUMENT and b"not device memory" in err()
        assert (out == 0).all()
        st.rays = 9
        assert go(renderer._scene, n=0) == N.PT_OK and st.rays == 0 and st.paths == 0
    finally:
        N.lib.pt_scene_destroy(fresh)
        N.lib.pt_scene_destroy(detached)
    a, _ = call(P, renderer, G.records(pts[:9], nrm[:9]), max_depth=0)
    b, _ = call(P, renderer, G.records(pts[:9], nrm[:9]), max_depth=8)
    assert same(a, b)
