"""-m gpu: pt_trace_rays (docs/SPEC.md §4.2) against the oracle on the same blob, on every layout and both builders.

Closest hits bit for bit (t bits and prim id equal pto_closest), the tmax rule at its boundary, occlusion, the visit counters,
barycentrics (against the float64 caster), the shared-edge leak, agreement with the render path's id images, batch sizes and
memory kinds, refused calls, and that queries leave progressive rendering untouched."""
import ctypes as C

import numpy as np
import pytest

import adversarial_scenes as S
import ray_caster64 as rc
from float64_support import CRACK_RAYS, PINNED_CRACKS, crack_rays
from trace_support import H, LAYOUTS, MISS, W, check_closest, commit, ids_of, oracle, ray_sets, records, same, scenes

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["cornell", "glass", "tess", "soup", "layers", "duplicates", "spheres64"])
def test_trace_matches_the_oracle(P, pto, renderer, name):
    """Every layout and builder, four ray sets: closest hits bit for bit, the visit counters (tmax = inf), the tmax rule at
    t_oracle, just below it and at random finite values, and occlusion."""
    N = P.native
    sd = scenes(P)[name]
    rng = np.random.default_rng(5)
    for width in LAYOUTS:
        for build in (0, N.PT_BVH_BUILD_LBVH):
            osc = commit(P, pto, renderer, sd, width | build)
            for rs, o, d in ray_sets(pto, sd):
                ctx = (name, width, build, rs)
                ids, ts, ost = oracle(pto, osc, o, d)
                rec = records(o, d)
                hits, st = renderer.TraceRays(rec, count_visits=True)
                check_closest(hits, ids, ts, ctx)
                assert st.rays == len(o)
                assert (st.node_visits, st.tri_tests, st.sphere_tests) == (ost.node_visits, ost.tri_tests, ost.sphere_tests), ctx
                hit = ids != MISS
                assert same(renderer.TraceRays(rec)[0], hits), ctx  # the plain kernel finds the same
                # tmax = t_oracle keeps the hit, the next float below it loses it
                tm = np.where(hit, ts, np.float32(1.0))
                h2, _ = renderer.TraceRays(rec, tmax=tm)
                assert np.array_equal(ids_of(h2)[hit], ids[hit]) and same(h2[hit], hits[hit]), ctx
                h3, _ = renderer.TraceRays(rec, tmax=np.nextafter(tm, np.float32(0)))
                assert (ids_of(h3)[hit] == MISS).all(), ctx
                # random finite tmax: the oracle's hit when t <= tmax, else a miss (SPEC §4.2)
                tr = (rng.random(len(o)) * 2.0 * np.where(hit, ts, 1.0)).astype(np.float32)
                h4, _ = renderer.TraceRays(rec, tmax=tr)
                keep = hit & (ts <= tr)
                check_closest(h4, np.where(keep, ids, MISS).astype(np.uint64), ts, ctx)
                # occlusion: occluded iff t_oracle <= tmax; a returned hit has t <= tmax and a valid id
                for tq in (np.float32(np.inf), tr):
                    h5, _ = renderer.TraceRays(rec, tmax=tq, occlusion=True)
                    occ = ids_of(h5) != MISS
                    want = hit & (ts <= tq)
                    assert np.array_equal(occ, want), ctx
                    n_prim = len(sd.tri_mat) + len(sd.sph_mat)
                    assert (ids_of(h5)[occ] < n_prim).all() and (h5[occ, 0] <= np.broadcast_to(tq, occ.shape)[occ]).all(), ctx
                    assert (h5[occ, 0] > 0).all() and (h5[:, 2:] == 0).all(), ctx


def test_tmax_degenerate_values_miss(P, pto, renderer):
    """tmax <= 0 and NaN give misses, in both query kinds."""
    sd = scenes(P)["glass"]
    commit(P, pto, renderer, sd, 0)
    o, d = rc.camera_rays(pto, sd.cam, W, H)
    for tm in (0.0, -0.0, -1.0, np.nan):
        for occlusion in (False, True):
            hits, _ = renderer.TraceRays(records(o, d), tmax=tm, occlusion=occlusion)
            assert (ids_of(hits) == MISS).all() and (hits[:, 0] == np.inf).all(), (tm, occlusion)


@pytest.mark.parametrize("name", ["tess", "glass"])
def test_barycentrics(P, pto, renderer, name):
    """Triangle hits: u, v >= 0, u + v <= 1, o + t d = v0 + u e1 + v e2 to float32 tolerance, and u, v equal the float64 caster's
    away from edges; sphere hits report 0, 0."""
    sd = scenes(P)[name]
    o, d = rc.camera_rays(pto, sd.cam, W, H)
    want, t64, edge, in_plane = rc.cast(sd.verts, sd.spheres, o, d)
    v = np.asarray(sd.verts, np.float64).reshape(-1, 3, 3)
    for width in (2, 68):
        commit(P, pto, renderer, sd, width)
        hits, _ = renderer.TraceRays((o, d))
        ids = ids_of(hits)
        tri = ids < len(v)
        u, w = hits[tri, 2].astype(np.float64), hits[tri, 3].astype(np.float64)
        assert tri.sum() > 0.5 * len(o)
        assert (u >= 0).all() and (w >= 0).all() and (u + w <= 1).all()
        j = ids[tri].astype(np.int64)
        p_ray = o[tri] + hits[tri, :1].astype(np.float64) * d[tri]
        p_tri = v[j, 0] + u[:, None] * (v[j, 1] - v[j, 0]) + w[:, None] * (v[j, 2] - v[j, 0])
        scale = np.abs(v).max()
        assert np.abs(p_ray - p_tri).max() <= 1e-5 * scale
        clear = tri.copy()
        clear[tri] = (want[tri] == ids[tri]) & (edge[tri] > 1e-4) & ~in_plane[tri]
        _, u64, w64, _ = rc._tri_eval(o[clear].astype(np.float64)[:, None], d[clear].astype(np.float64)[:, None],
                                      v[ids[clear].astype(np.int64), 0][:, None], (v[ids[clear].astype(np.int64), 1] - v[ids[clear].astype(np.int64), 0])[:, None],
                                      (v[ids[clear].astype(np.int64), 2] - v[ids[clear].astype(np.int64), 0])[:, None])
        assert clear.sum() > 0.4 * len(o)
        assert np.abs(hits[clear, 2] - u64[:, 0]).max() <= 1e-4 and np.abs(hits[clear, 3] - w64[:, 0]).max() <= 1e-4
        sph = (ids >= len(v)) & (ids != MISS)
        assert (hits[sph, 2:] == 0).all()


def test_shared_edge_rays_in_one_call(P, pto, renderer):
    """The 300 shared-edge rays of test_shared_edge_leak_is_pinned in one call: misses exactly where the oracle misses, on both
    builders (the closest-hit query is what the watertight change will be checked with)."""
    sd, _, o, d = crack_rays(P, pto)
    bf = pto.Scene(sd)
    want = np.array([bf.closest(o[i], d[i])[0] for i in range(CRACK_RAYS)], np.uint64)
    assert int((want == MISS).sum()) == PINNED_CRACKS
    for build in (0, P.native.PT_BVH_BUILD_LBVH):
        renderer.SetScene(sd, build)
        hits, _ = renderer.TraceRays((o, d))
        assert np.array_equal(ids_of(hits), want), build


def test_same_ids_as_the_render_path(P, pto, renderer):
    """Camera rays of an id scene: the query's prim ids equal the id image that pt_render makes of the same scene."""
    for sd in (scenes(P)["glass"], scenes(P)["tess"]):
        ids = S.id_scene(sd)
        o, d = rc.camera_rays(pto, ids.cam, W, H)
        for width in LAYOUTS:
            renderer.SetScene(ids, width)
            renderer.Params = S.params_id(W, H)
            renderer.Render(0.0)
            image = S.ids_of(renderer.ReadFramebuffer())
            hits, _ = renderer.TraceRays((o, d))
            assert np.array_equal(ids_of(hits), image), width


def test_sizes_and_memory_kinds(P, pto, renderer):
    """n = 1, 63, 65 and a 4M-ray batch (past the 2^20-lane grid: lanes reuse their overflow columns, on a scene whose every ray
    spills out of LDS); torch device tensors and numpy host arrays give identical hits."""
    import torch
    sd = scenes(P)["layers"]
    osc = commit(P, pto, renderer, sd, 68)
    assert renderer.BvhInfo().stack_need > 12
    o, d = rc.camera_rays(pto, sd.cam, W, H)
    ids, ts, _ = oracle(pto, osc, o, d)
    rec = records(o, d)
    for n in (1, 63, 65):
        hits, st = renderer.TraceRays(rec[:n])
        check_closest(hits, ids[:n], ts[:n], n)
        dh, _ = renderer.TraceRays(torch.from_numpy(rec[:n]).cuda())
        assert same(dh.cpu().numpy(), hits) and st.rays == n
    reps = -(-(4 << 20) // len(rec))
    big = np.tile(rec, (reps, 1))
    hits, st = renderer.TraceRays(big)
    assert st.rays == len(big) >= 4 << 20 and st.gpu_ms > 0
    assert same(hits, np.tile(renderer.TraceRays(rec)[0], (reps, 1)))
    check_closest(hits[-len(rec):], ids, ts, "big")
    dh, _ = renderer.TraceRays(torch.from_numpy(big).cuda())
    assert same(dh.cpu().numpy(), hits)
    dh, _ = renderer.TraceRays((torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()), occlusion=True)
    assert same(dh.cpu().numpy(), renderer.TraceRays((o, d), occlusion=True)[0])


def test_refused_calls(P, pto, renderer):
    """Misaligned device pointers, unknown flags, OCCLUSION | COUNT_VISITS and an uncommitted scene are refused with the documented
    status; n_rays == 0 is a no-op."""
    import torch
    N = P.native
    sd = scenes(P)["cornell"]
    commit(P, pto, renderer, sd, 0)
    o, d = rc.camera_rays(pto, sd.cam, W, H)
    rays = torch.from_numpy(records(o, d)).cuda()
    hits = torch.zeros((len(o) + 1, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx, scene, st = renderer._ctx, renderer._scene, N.pt_stats()
    call = lambda r, h, n, f, s=scene: N.lib.pt_trace_rays(ctx, s, C.c_void_p(r), C.c_void_p(h), n, f, C.byref(st))
    rp, hp = rays.data_ptr(), hits.data_ptr()
    assert call(rp, hp, len(o), 0) == N.PT_OK
    assert call(rp + 4, hp, len(o) - 1, 0) == N.PT_ERR_INVALID_ARGUMENT
    assert call(rp, hp + 8, len(o), 0) == N.PT_ERR_INVALID_ARGUMENT
    assert call(rp, hp, len(o), 8) == N.PT_ERR_INVALID_ARGUMENT
    assert call(rp, hp, len(o), N.PT_TRACE_OCCLUSION | N.PT_TRACE_COUNT_VISITS) == N.PT_ERR_INVALID_ARGUMENT
    before = hits.clone()
    st.rays = 99
    assert call(rp, hp, 0, 0) == N.PT_OK and st.rays == 0
    assert torch.equal(hits.view(torch.int32), before.view(torch.int32))
    fresh = C.c_void_p()
    assert N.lib.pt_scene_create(ctx, C.byref(fresh)) == N.PT_OK
    try:
        assert call(rp, hp, len(o), 0, fresh) == N.PT_ERR_NOT_COMMITTED
    finally:
        N.lib.pt_scene_destroy(fresh)
    with pytest.raises(P.PtException):
        renderer.TraceRays(records(o, d), occlusion=True, count_visits=True)


def test_queries_between_progressive_frames(P, pto, renderer):
    """A progressive sequence (PT_FLAG_ACCUMULATE, 8 streams, offsets 0, 4, 8) and a restart at 0 with queries between every two
    frames: every frame equals the same sequence without queries, and the oracle's."""
    N = P.native
    sd = scenes(P)["glass"]
    osc = commit(P, pto, renderer, sd, 0)
    o, d = rc.camera_rays(pto, sd.cam, W, H)
    big = np.tile(records(o, d), (64, 1))
    seq = [(0, 0), (4, N.PT_FLAG_ACCUMULATE), (8, N.PT_FLAG_ACCUMULATE), (0, 0)]

    def run(queries):
        frames = []
        for offset, flags in seq:
            if queries:
                renderer.TraceRays(big)
                renderer.TraceRays(big, occlusion=True, tmax=0.5)
            renderer.Params = P.make_params(W, H, spp=4, max_depth=8, streams=8, sample_offset=offset, flags=flags)
            renderer.Render(0.0)
            frames.append(renderer.ReadFramebuffer())
        return frames

    plain, mixed = run(False), run(True)
    for k, (a, b) in enumerate(zip(plain, mixed)):
        assert np.array_equal(a, b), k
    for k, spp in ((2, 12), (3, 4)):
        ref, _ = pto.render(osc, P.make_params(W, H, spp=spp, max_depth=8, streams=8))
        assert np.array_equal(mixed[k], ref), k
