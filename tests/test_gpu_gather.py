"""-m gpu: pt_gather (include/ptrt.h, docs/SPEC.md §12) against tests/gather_ref.py.

The points are the first hits of a 24 x 18 camera frame (gather_ref.case), K = 64 and ray_eps = 1e-3 unless a test says otherwise. The count
of visible samples, round(visibility * K), is compared exactly; E and bent within (K + 2) * 2^-24 — the bound of a sum of K f32 terms in
any order ((K - 1) roundings) plus the division by K and the conversion of the result, relative to sum |term| / K for E and absolute for
bent, whose terms are unit vectors. Every test commits its own scene on the session's renderer."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import env_checker
import gather_ref as G
from gather_device import K, LBVH, SENTINEL, SKY, call, other_state_is_untouched, same

pytestmark = pytest.mark.gpu


def bound(samples):
    return (samples + 2) * 2.0 ** -24


def gather(P, r, rec, **kw):
    """pt_gather on (n, 8) records (gather_device.call): (out (n, 8) float32, pt_stats)."""
    return call(P, r, rec, paths=False, **kw)


def counts_of(out, samples):
    c = np.rint(out[:, 3].astype(np.float64) * samples).astype(np.int64)
    assert np.array_equal((c / samples).astype(np.float32), out[:, 3]), "visibility is not count / K"
    return c


def check(out, ref, samples, ctx):
    """Every record of `out` against the reference dict of gather_ref.gather."""
    assert np.isfinite(out).all() and (out[:, 7] == 0).all(), ctx
    valid = ref["visibility"] >= 0
    got = counts_of(out[valid], samples)
    assert np.array_equal(got, ref["count"][valid]), (ctx, np.nonzero(got != ref["count"][valid])[0][:8])
    b = bound(samples)
    errE = np.abs(out[valid, 0:3].astype(np.float64) - ref["E"][valid])
    print(f"{ctx}: max |dE| / (sum|term|/K) = {(errE / np.maximum(ref['absE'][valid], 1e-300)).max():.3e}, "
          f"max |dbent| = {np.abs(out[valid, 4:7] - ref['bent'][valid]).max():.3e}, bound {b:.3e}")
    assert (errE <= b * ref["absE"][valid]).all(), ctx
    assert (np.abs(out[valid, 4:7].astype(np.float64) - ref["bent"][valid]) <= b).all(), ctx
    assert (out[~valid] == SENTINEL).all(), ctx


@pytest.fixture(scope="module")
def glass(P, pto):
    return G.case(P, pto, "glass")


@pytest.fixture(scope="module")
def tess(P, pto):
    return G.case(P, pto, "tess")


def test_counts_are_exact_on_every_layout(P, pto, renderer, glass, tess):
    """1. The visible-sample count of every point equals the reference's, unbounded and with max_distance about half the box, on
    Cornell-glass (BVH2) and on the 2000-triangle Cornell under every layout and the GPU builder; all layouts give the same bits."""
    sd, pts, nrm, rays = glass
    rec = G.records(pts, nrm)
    renderer.SetScene(dataclasses.replace(sd, sky=SKY), 2)
    seen = 0
    for md in (0.0, G.half_box(sd)):
        out, st = gather(P, renderer, rec, max_distance=md)
        ref = G.gather(rays, md, sky=SKY)
        check(out, ref, K, ("glass", md))
        assert st.paths == len(rec) and st.rays == K * len(rec) and st.gpu_ms > 0 and st.node_visits == 0 and st.iterations == 0
        seen += int(ref["count"].sum())
    sd, pts, nrm, rays = tess
    rec = G.records(pts, nrm)
    refs = {md: G.gather(rays, md, sky=SKY) for md in (0.0, G.half_box(sd))}
    assert 0 < refs[0.0]["count"].sum() < refs[G.half_box(sd)]["count"].sum() < K * len(rec) and seen > 0
    first = {}
    for width in (2, 4, 68, 72, 73, 68 | LBVH):
        renderer.SetScene(dataclasses.replace(sd, sky=SKY), width)
        for md, ref in refs.items():
            out, _ = gather(P, renderer, rec, max_distance=md)
            check(out, ref, K, ("tess", width, md))
            assert same(out, first.setdefault(md, out)), ("layouts differ", width, md)


def test_sums_with_a_sky_and_with_a_map(P, pto, renderer, glass):
    """2. E and bent within the bound, with the constant sky (1, 2, 3) and with a map whose every texel has its own colour; with the
    constant sky E is visibility * sky within the same bound — in particular on open (visibility 1) and enclosed (0) points."""
    sd, pts, nrm, rays = glass
    rec = G.records(pts, nrm)
    renderer.SetScene(dataclasses.replace(sd, sky=SKY), 0)
    out, _ = gather(P, renderer, rec)
    ref = G.gather(rays, 0.0, sky=SKY)
    check(out, ref, K, "sky")
    want = out[:, 3:4].astype(np.float64) * SKY.astype(np.float64)
    assert (np.abs(out[:, 0:3] - want) <= bound(K) * np.abs(want)).all()
    assert (out[out[:, 3] == 0][:, 0:3] == 0).all()
    # a short max_distance opens every point: E is the sky itself
    out, _ = gather(P, renderer, rec, max_distance=1e-4)
    check(out, G.gather(rays, 1e-4, sky=SKY), K, "open")
    assert (out[:, 3] == 1).all() and (np.abs(out[:, 0:3] - SKY) <= bound(K) * SKY).all()
    env = env_checker.distinct(8)
    renderer.SetScene(dataclasses.replace(sd, sky=SKY, environment=env), 0)
    L = G.radiance(rays, env=env)
    for md in (0.0, G.half_box(sd)):
        out, _ = gather(P, renderer, rec, max_distance=md)
        check(out, G.gather(rays, md, L=L), K, ("map", md))
    assert len(np.unique(L.reshape(-1, 3), axis=0)) > 32  # the directions reach most of the upper and lower texels


def test_extremes(P, pto, renderer):
    """3. A point above a single ground triangle facing up sees everything (exactly 1); a point inside the closed box sees nothing
    (exactly 0), and everything once max_distance is shorter than the way to any wall."""
    sd = G.scene(P, "closed")
    ground = dataclasses.replace(sd, verts=np.array([[-50.0, 0.0, -50.0, 50.0, 0.0, -50.0, 0.0, 0.0, 90.0]], np.float32),
                                 tri_mat=np.zeros(1, np.uint32), sky=SKY)
    renderer.SetScene(ground, 0)
    out, st = gather(P, renderer, G.records(np.array([[0.0, 0.5, 0.0]], np.float32), np.array([[0.0, 3.0, 0.0]], np.float32)))
    assert out[0, 3] == 1.0 and st.rays == K
    assert np.abs(out[0, 0:3] - SKY).max() <= bound(K) * 3 and out[0, 5] > 0.5
    v = np.asarray(sd.verts, np.float32).reshape(-1, 3)
    centre = (0.5 * (v.min(0) + v.max(0)))[None].astype(np.float32)
    up = np.array([[0.0, 1.0, 0.0]], np.float32)
    from float64_support import build_bvh_detached
    info, nodes, tris = build_bvh_detached(sd, 68)
    assert G.gather(G.rays(P, pto, pto.Scene(sd, (info.width, nodes, tris)), centre, up), 0.0, sky=SKY)["count"][0] == 0  # it is closed
    renderer.SetScene(dataclasses.replace(sd, sky=SKY), 0)
    out, _ = gather(P, renderer, G.records(centre, up))
    assert same(out, np.zeros((1, 8), np.float32))
    out, _ = gather(P, renderer, G.records(centre, up), max_distance=1e-4)
    assert out[0, 3] == 1.0


@pytest.fixture(scope="module")
def shape_rays(P, pto, glass):
    """The reference rays of the first 257 points with 100 samples each: sample k of point i is the same ray whatever K and n are."""
    from float64_support import build_bvh_detached
    sd, pts, nrm, _ = glass
    info, nodes, tris = build_bvh_detached(sd, 68)
    osc = pto.Scene(sd, (info.width, nodes, tris))
    return osc, G.rays(P, pto, osc, pts[:257], nrm[:257], 100)


def cut(r, n, samples):
    return G.Rays(r.valid[:n], r.o[:n], r.d[:n, :samples], r.ids[:n, :samples], r.t[:n, :samples])


@pytest.mark.parametrize("samples", [1, 3, 64, 100])
def test_shapes(P, pto, renderer, glass, shape_rays, samples):
    """4. n_points in {1, 63, 65, 257} x K: groups of 1, 4 and 64 lanes, several samples per lane (100), partial last waves, more than
    one workgroup. Every record is right and a guard band behind `out` keeps its bytes."""
    import torch
    N = P.native
    sd, pts, nrm, _ = glass
    renderer.SetScene(dataclasses.replace(sd, sky=SKY), 0)
    for n in (1, 63, 65, 257):
        rec = G.records(pts[:n], nrm[:n])
        d_rec = torch.as_tensor(rec, device="cuda")
        d_out = torch.full((n + 16, 8), 7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        gp = N.pt_gather_params(samples=samples, ray_eps=G.EPS)
        st = N.pt_stats()
        assert N.lib.pt_gather(renderer._ctx, renderer._scene, C.c_void_p(d_rec.data_ptr()), C.c_void_p(d_out.data_ptr()), n, C.byref(gp),
                               C.byref(st)) == N.PT_OK, N.lib.pt_last_error(renderer._ctx)
        out = d_out.cpu().numpy()
        assert (out[n:] == 7.0).all(), ("guard band", n, samples)
        check(out[:n], G.gather(cut(shape_rays[1], n, samples), 0.0, sky=SKY), samples, ("shape", n, samples))
        assert st.rays == n * samples and st.paths == n


def test_4096_samples(P, pto, renderer, glass, shape_rays):
    """4. The largest K on 8 points: 64 samples per lane."""
    sd, pts, nrm, _ = glass
    idx = np.arange(8) * 37  # spread over the frame
    renderer.SetScene(dataclasses.replace(sd, sky=SKY), 0)
    out, st = gather(P, renderer, G.records(pts[idx], nrm[idx]), samples=4096, host=False)
    # point j of the call has key index j, not idx[j]: the reference takes the same points in the same places
    ref = G.gather(G.rays(P, pto, shape_rays[0], pts[idx], nrm[idx], 4096), 0.0, sky=SKY)
    check(out, ref, 4096, "K=4096")
    assert st.rays == 8 * 4096 and 0 < ref["count"].sum() < 8 * 4096


def test_merge_and_split(P, pto, renderer, glass):
    """5. Sample ranges merge, point ranges split, device and host memory agree, and a call repeats itself bit for bit."""
    sd, pts, nrm, _ = glass
    rec = G.records(pts, nrm)
    renderer.SetScene(dataclasses.replace(sd, sky=SKY), 0)
    whole, _ = gather(P, renderer, rec)
    lo, _ = gather(P, renderer, rec, samples=32)
    hi, _ = gather(P, renderer, rec, samples=32, sample_offset=32)
    assert np.array_equal(counts_of(lo, 32) + counts_of(hi, 32), counts_of(whole, K))
    assert np.abs((lo[:, 4:7].astype(np.float64) + hi[:, 4:7]) / 2 - whole[:, 4:7]).max() <= bound(K)
    h = len(rec) // 2 + 1
    for samples in (K, 16):  # 16: four points per wave, and the cut falls inside a wave of the whole call
        assert samples == K or h % 4 != 0
        one, _ = gather(P, renderer, rec, samples=samples)
        a, _ = gather(P, renderer, rec[:h], samples=samples)
        b, _ = gather(P, renderer, rec[h:], samples=samples, point_offset=h)
        assert same(np.concatenate([a, b]), one) and (samples != K or same(one, whole))
    dev, _ = gather(P, renderer, rec, host=False)
    again, _ = gather(P, renderer, rec)
    assert same(dev, whole) and same(again, whole)
    other, _ = gather(P, renderer, rec, seed=1)
    assert not same(other, whole)


def test_invalid_points(P, pto, renderer, glass):
    """6. A NaN position, an infinite normal and a zero normal give the sentinel rows and trace nothing; their neighbours in the same
    wave (4 points per wave at K = 16) and everywhere else are what they are without them; stats.rays leaves them out."""
    sd, pts, nrm, _ = glass
    rec = G.records(pts[:70], nrm[:70])
    renderer.SetScene(dataclasses.replace(sd, sky=SKY), 0)
    bad = rec.copy()
    bad[5, 1] = np.nan
    bad[6, 4] = np.inf
    bad[41, 4:7] = 0.0
    for samples in (16, K):
        clean, st0 = gather(P, renderer, rec, samples=samples)
        out, st = gather(P, renderer, bad, samples=samples)
        ok = np.ones(70, bool)
        ok[[5, 6, 41]] = False
        assert same(out[ok], clean[ok]) and (out[~ok] == SENTINEL).all() and np.isfinite(out).all()
        assert st0.rays == 70 * samples and st.rays == 67 * samples and st.paths == 70
    # normals of any length are normalised; a subnormal-length normal whose dot underflows to 0 is invalid
    scaled = rec.copy()
    scaled[:, 4:7] *= 4.0
    out, _ = gather(P, renderer, scaled)
    clean, _ = gather(P, renderer, rec)
    assert np.array_equal(counts_of(out, K), counts_of(clean, K))
    tiny = rec[:1].copy()
    tiny[0, 4:7] = (1e-30, 0.0, 0.0)
    out, st = gather(P, renderer, tiny)
    assert (out[0] == SENTINEL).all() and st.rays == 0


def test_other_state_is_untouched(P, pto, glass):
    """7. A PT_FLAG_ACCUMULATE sequence with a pt_gather in the middle is the sequence without it, and the displayed and denoised
    images, the guides and the temporal history of the frame survive the call."""
    sd, pts, nrm, _ = glass
    other_state_is_untouched(P, sd, G.records(pts, nrm), paths=False)


def test_refusals_that_need_a_context(P, pto, renderer, glass):
    """The checks behind the ones tests/test_gather.py can reach without a device, in their order: alignment, the scene's context,
    commit, the batch size; and an empty batch is fine."""
    N = P.native
    sd, pts, nrm, _ = glass
    renderer.SetScene(sd, 0)
    rec = np.zeros((5, 8), np.float32)
    rec[:, 5] = 1.0
    out = np.zeros((5, 8), np.float32)
    st = N.pt_stats()
    ctx = renderer._ctx
    err = lambda: N.lib.pt_last_error(ctx)

    def call(scene, p_off=0, o_off=0, n=4, flags=N.PT_GATHER_HOST_MEMORY, gp=None):
        gp = gp or N.pt_gather_params(samples=4, flags=flags)
        return N.lib.pt_gather(ctx, scene, C.c_void_p(rec.ctypes.data + p_off), C.c_void_p(out.ctypes.data + o_off), n, C.byref(gp), C.byref(st))

    fresh = C.c_void_p()
    assert N.lib.pt_scene_create(ctx, C.byref(fresh)) == N.PT_OK
    detached = C.c_void_p()
    assert N.lib.pt_scene_create(None, C.byref(detached)) == N.PT_OK
    try:
        assert call(fresh, p_off=2) == N.PT_ERR_INVALID_ARGUMENT and b"4-byte aligned" in err()       # before the commit check
        assert call(fresh, o_off=4, flags=0) == N.PT_ERR_INVALID_ARGUMENT and b"16-byte aligned" in err()
        assert call(detached, n=1 << 32) == N.PT_ERR_INVALID_ARGUMENT and b"another context" in err()   # before the batch size
        assert call(fresh, n=1 << 32) == N.PT_ERR_NOT_COMMITTED and b"not committed" in err()
        assert call(renderer._scene, n=1 << 32) == N.PT_ERR_INVALID_ARGUMENT and b"batch size" in err()
        assert call(renderer._scene, flags=0) == N.PT_ERR_INVALID_ARGUMENT and b"not device memory" in err()
        assert (out == 0).all()
        st.rays = 9
        assert call(renderer._scene, n=0) == N.PT_OK and st.rays == 0 and st.paths == 0
        assert call(renderer._scene, gp=N.pt_gather_params(samples=0, flags=N.PT_GATHER_HOST_MEMORY)) == N.PT_OK and st.rays == 4 * 64
    finally:
        N.lib.pt_scene_destroy(fresh)
        N.lib.pt_scene_destroy(detached)


def test_renderer_gather_takes_numpy_and_torch(P, pto, renderer, glass):
    """Renderer.Gather: numpy arrays through the staged path, device tensors as device pointers, the same bits either way."""
    import torch
    sd, pts, nrm, rays = glass
    renderer.SetScene(dataclasses.replace(sd, sky=SKY), 0)
    E, vis, bent, st = renderer.Gather(pts, nrm, samples=K, ray_eps=G.EPS)
    check(np.concatenate([E, vis[:, None], bent, np.zeros((len(pts), 1), np.float32)], 1), G.gather(rays, 0.0, sky=SKY), K, "Renderer.Gather")
    tE, tvis, tbent, tst = renderer.Gather(torch.as_tensor(pts, device="cuda"), torch.as_tensor(nrm, device="cuda"), samples=K, ray_eps=G.EPS)
    assert tE.is_cuda and same(tE.cpu().numpy(), E) and same(tvis.cpu().numpy(), vis) and same(tbent.cpu().numpy(), bent)
    assert st.rays == tst.rays == K * len(pts)
