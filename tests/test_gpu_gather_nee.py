"""-m gpu: pt_gather_paths with PT_GATHER_PATHS_NEXT_EVENT (include/ptrt.h, docs/SPEC.md §12.2) against the scalar checker of
tests/gather_nee_ref/.

Every comparison is bit for bit — the eight floats of every record and pt_stats::rays (segments + shadow rays). The points are the first
hits of a 24 x 18 camera frame (gather_ref.first_hits), K = 64 and ray_eps = 1e-3 unless a test says otherwise. Every test commits its
own scene on the session's renderer."""
import dataclasses

import numpy as np
import pytest

import env_checker
import gather_nee_checker as GN
import gather_paths_checker as GP
import gather_ref as G
import nee_checker as nc
from gather_device import K, LBVH, SENTINEL, bits, same

pytestmark = pytest.mark.gpu


def held(P, r, osc, pts, nrm, ctx, env=None, host=True, ref=None, **kw):
    """One flagged call on the device and the checker's: the same bits, the same rays. Returns the device's (out, stats) and the
    checker's result (ref: one made earlier for the same arguments)."""
    out, st = GN.call(P, r, G.records(pts, nrm), host=host, **{"ray_eps": G.EPS, **kw})
    ref = ref or GN.gather(osc, pts, nrm, env=env, **{"ray_eps": G.EPS, **kw})
    bad = np.nonzero((bits(out) != bits(ref.rows)).any(1))[0]
    assert len(bad) == 0, (ctx, len(bad), bad[:4], out[bad[:2]], ref.rows[bad[:2]])
    assert st.rays == ref.rays and st.paths == len(pts), (ctx, st.rays, ref.segments, ref.shadow_rays)
    assert np.isfinite(out).all()
    return out, st, ref


def _case(P, pto, sd):
    pts, nrm = G.first_hits(P, pto, sd)
    osc = pto.Scene(sd)
    osc.build_own_bvh()
    return sd, pts, nrm, osc


@pytest.fixture(scope="module")
def glass(P, pto):
    return _case(P, pto, G.scene(P, "glass"))


@pytest.fixture(scope="module")
def tess(P, pto):
    return _case(P, pto, G.scene(P, "tess"))


@pytest.fixture(scope="module")
def lights(P, pto):
    return _case(P, pto, nc.many_lights_scene(P, G.W, G.H))


DEPTHS = ((8, 3), (2, 3), (1, 0))


def test_layouts(P, pto, renderer, glass, tess):
    """1. Cornell-glass (Lambert, metal, dielectric, spheres, the emissive quad) on BVH2 and the 2000-triangle Cornell under every layout
    and the GPU builder, with max_depth 8, 2 and 1: the checker's bits and rays, and so the same on every layout."""
    sd, pts, nrm, osc = glass
    assert len(pts) >= 257 and len(sd.spheres) > 0 and {int(k) for k in sd.mats["kind"]} >= {0, 1, 2} and sd.mats["emission"].any()
    renderer.SetScene(sd, 2)
    for md, rr in DEPTHS:
        out, st, ref = held(P, renderer, osc, pts, nrm, ("glass", md), max_depth=md, rr_start=rr)
        assert (out[:, 0:3] > 0).any() and ref.shadow_rays > 0 and st.gpu_ms > 0
    sd, pts, nrm, osc = tess
    first, refs = {}, {}
    for width in (2, 4, 68, 72, 73, 68 | LBVH):
        renderer.SetScene(sd, width)
        for md, rr in DEPTHS:
            out, _, refs[md] = held(P, renderer, osc, pts, nrm, ("tess", width, md), ref=refs.get(md), max_depth=md, rr_start=rr)
            assert same(out, first.setdefault(md, out)), ("layouts differ", width, md)


@pytest.mark.parametrize("samples", [1, 5, 32, 100])
def test_group_shapes(P, pto, renderer, lights, samples):
    """2. K of 1, 5, 32 and 100 on 1, 65 and all points of the many-lights scene: 64 points per wave, lanes with g >= K, and lanes that
    start their next sample in place while their neighbours wait for a shadow ray."""
    sd, pts, nrm, osc = lights
    renderer.SetScene(sd, 0)
    for n in (1, 65, len(pts)):
        held(P, renderer, osc, pts[:n], nrm[:n], ("shape", n, samples), samples=samples)


def test_depth_and_roulette(P, pto, renderer, glass):
    """3. max_depth 255 with rr_start 0 and 255, max_depth 8 with rr_start 8 and 0, max_depth 0 (= 8); at max_depth 1 rays is K x points
    plus the checker's shadow rays."""
    sd, pts, nrm, osc = glass
    renderer.SetScene(sd, 0)
    for md, rr in ((255, 0), (255, 255), (8, 8), (8, 0), (0, 3), (1, 0)):
        out, st, ref = held(P, renderer, osc, pts, nrm, ("depth", md, rr), max_depth=md, rr_start=rr)
        assert md != 1 or (ref.segments == K * len(pts) and st.rays == K * len(pts) + ref.shadow_rays)


def test_light_kinds_and_consequences(P, pto, renderer, glass):
    """4. and 5. On the same geometry: triangle lights only, a lit map only (emission removed), both, and an all-black map with the
    triangles (psel = 1): each the checker's, and they differ where they should. Against the unflagged call on the same renderer:
    visibility and bent are its bits for max_distance 0, half the box and 1e-4, and rays(flagged) - rays(unflagged) is the checker's
    shadow-ray count; with no light of either kind the whole record and rays are the unflagged call's."""
    sd, pts, nrm, osc = glass
    rec = G.records(pts, nrm)
    env, black = env_checker.distinct(8), np.zeros((8, 8, 3), np.float32)
    dark = GP.without_emission(sd)
    dosc = pto.Scene(dark)
    dosc.build_own_bvh()
    outs = {}
    for name, scene, o, e in (("triangles", sd, osc, None), ("map", dark, dosc, env), ("both", sd, osc, env), ("black map", sd, osc, black)):
        renderer.SetScene(scene if e is None else dataclasses.replace(scene, environment=e), 0)
        outs[name], st, ref = held(P, renderer, o, pts, nrm, name, env=e)
        assert ref.shadow_rays > 0 and ref.lit == (name in ("map", "both")) and (ref.n_lights > 0) == (name != "map")
        plain, pst = GN.call(P, renderer, rec, next_event=False, ray_eps=G.EPS)
        assert st.rays - pst.rays == ref.shadow_rays and pst.rays == ref.segments, (name, st.rays, pst.rays, ref.shadow_rays)
        assert same(outs[name][:, 3:], plain[:, 3:]) and not same(outs[name][:, :3], plain[:, :3]), name
        for dist in (G.half_box(sd), 1e-4):
            a, _ = GN.call(P, renderer, rec, max_distance=dist, ray_eps=G.EPS)
            b, _ = GN.call(P, renderer, rec, next_event=False, max_distance=dist, ray_eps=G.EPS)
            assert same(a[:, 3:], b[:, 3:]) and same(a[:, :3], outs[name][:, :3]), (name, dist)  # shadow rays and paths ignore max_distance
    names = list(outs)
    assert not np.asarray(sd.sky).any()  # so a black map is this scene's sky: with psel = 1 the ENV kernel gives the plain kernel's bits
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert same(outs[a], outs[b]) == ((a, b) == ("triangles", "black map")), (a, b)
    for e in (None, black):  # no light of either kind: the unflagged call, kernel and all
        renderer.SetScene(dataclasses.replace(dark, sky=np.array([1.0, 2.0, 3.0], np.float32)) if e is None else dataclasses.replace(dark, environment=e), 0)
        a, sa = GN.call(P, renderer, rec, ray_eps=G.EPS)
        b, sb = GN.call(P, renderer, rec, next_event=False, ray_eps=G.EPS)
        assert same(a, b) and sa.rays == sb.rays


def test_split_and_merge(P, pto, renderer, lights):
    """6. A bake split by point_offset, the cut inside a wave at K = 16, is the unsplit bake; a call repeats itself; another seed is another
    bake."""
    sd, pts, nrm, osc = lights
    rec = G.records(pts, nrm)
    renderer.SetScene(sd, 0)
    h = len(rec) // 2 + 1
    for samples in (K, 16):
        assert samples == K or h % 4 != 0
        one, s1 = GN.call(P, renderer, rec, samples=samples, ray_eps=G.EPS)
        a, sa = GN.call(P, renderer, rec[:h], samples=samples, ray_eps=G.EPS)
        b, sb = GN.call(P, renderer, rec[h:], samples=samples, point_offset=h, ray_eps=G.EPS)
        assert same(np.concatenate([a, b]), one) and sa.rays + sb.rays == s1.rays
    again, s2 = GN.call(P, renderer, rec, samples=16, ray_eps=G.EPS)
    other, _ = GN.call(P, renderer, rec, samples=16, seed=1, ray_eps=G.EPS)
    assert same(again, one) and s2.rays == s1.rays and not same(other, one)


def test_edge_inputs(P, pto, renderer, glass):
    """7. Invalid points among valid ones give the sentinel rows, trace nothing and leave their neighbours in the wave alone (4 points per
    wave at K = 16); the grazing scene at ray_eps 0; points on the lights themselves, facing both ways: finite, and the checker's bits."""
    sd, pts, nrm, osc = glass
    renderer.SetScene(sd, 0)
    bad_p, bad_n = pts[:70].copy(), nrm[:70].copy()
    bad_p[5, 1] = np.nan
    bad_n[6, 0] = np.inf
    bad_n[41] = 0.0
    ok = np.ones(70, bool)
    ok[[5, 6, 41]] = False
    for samples in (16, K):
        clean, st0 = GN.call(P, renderer, G.records(pts[:70], nrm[:70]), samples=samples, ray_eps=G.EPS)
        out, st, _ = held(P, renderer, osc, bad_p, bad_n, ("invalid", samples), samples=samples)
        assert same(out[ok], clean[ok]) and (out[~ok] == SENTINEL).all() and st.rays < st0.rays
    gz = nc.grazing_scene(P, G.W, G.H)
    gpts, gnrm = G.first_hits(P, pto, gz)
    gosc = pto.Scene(gz)
    gosc.build_own_bvh()
    renderer.SetScene(gz, 0)
    held(P, renderer, gosc, gpts, gnrm, "grazing, eps 0", ray_eps=0.0)
    v = np.asarray(gz.verts, np.float32).reshape(-1, 3, 3)
    on = v[gz.mats["emission"].any(1)[gz.tri_mat]]
    lp = np.concatenate([on.mean(1), on[:, 0], 0.5 * (on[:, 0] + on[:, 1])])
    ln = np.cross(on[:, 1] - on[:, 0], on[:, 2] - on[:, 0])
    ln = np.tile(ln / np.linalg.norm(ln, axis=1, keepdims=True), (3, 1)).astype(np.float32)
    lp, ln = G.both_sides(lp, ln)
    for eps in (G.EPS, 0.0):
        held(P, renderer, gosc, lp, ln, ("on the lights", eps), ray_eps=eps)


def test_updates_move_the_lights(P, pto, renderer):
    """8. After pt_scene_update_triangles moves and resizes the light quad, from host and from device memory, the flagged call equals that
    of a fresh commit of the moved geometry, and the checker's."""
    import torch
    sd = env_checker.scene(P, "cornell", G.W, G.H)
    pts, nrm = G.first_hits(P, pto, sd)
    light = np.nonzero(sd.mats["emission"].sum(axis=1)[sd.tri_mat] > 0)[0]
    v2 = sd.verts.copy()
    q = v2[light].reshape(-1, 3, 3)
    q[:, :, 0] = q[:, :, 0] * 1.5 + 0.2   # wider, off centre
    q[:, :, 1] -= 0.3                      # lower
    v2[light] = q.reshape(-1, 9)
    moved = dataclasses.replace(sd, verts=v2)
    mosc = pto.Scene(moved)
    mosc.build_own_bvh()
    ref = None
    for width in (2, 68 | LBVH):
        renderer.SetScene(moved, width)
        fresh, _, ref = held(P, renderer, mosc, pts, nrm, ("fresh", width), ref=ref)
        for verts in (v2, torch.from_numpy(v2).cuda()):
            renderer.SetScene(sd, width)
            before, _ = GN.call(P, renderer, G.records(pts, nrm), ray_eps=G.EPS)
            renderer.UpdateGeometry(verts=verts)
            out, _, _ = held(P, renderer, mosc, pts, nrm, ("updated", width, type(verts)), ref=ref)
            assert same(out, fresh) and not same(before, fresh)


def test_interface_and_stats(P, pto, renderer, glass):
    """9. Host and device memory give the same bits; Renderer.GatherPaths(next_event=True) takes numpy arrays and device tensors; the
    stats fields other than rays, paths and gpu_ms are 0."""
    import torch
    sd, pts, nrm, osc = glass
    renderer.SetScene(sd, 0)
    out, st, ref = held(P, renderer, osc, pts, nrm, "host")
    dev, sd_, _ = held(P, renderer, osc, pts, nrm, "device", host=False, ref=ref)
    assert same(dev, out) and sd_.rays == st.rays
    assert st.paths == len(pts) and st.gpu_ms > 0
    for f in ("node_visits", "tri_tests", "sphere_tests", "iterations"):
        assert getattr(st, f) == 0, f
    E, vis, bent, rst = renderer.GatherPaths(pts, nrm, samples=K, ray_eps=G.EPS, max_depth=8, rr_start=3, next_event=True)
    assert same(np.concatenate([E, vis[:, None], bent], 1), out[:, :7]) and rst.rays == st.rays
    tE, tvis, tbent, tst = renderer.GatherPaths(torch.as_tensor(pts, device="cuda"), torch.as_tensor(nrm, device="cuda"), samples=K, ray_eps=G.EPS,
                                                max_depth=8, rr_start=3, next_event=True)
    assert tE.is_cuda and same(tE.cpu().numpy(), E) and same(tvis.cpu().numpy(), vis) and same(tbent.cpu().numpy(), bent) and tst.rays == st.rays
    pE, _, _, pst = renderer.GatherPaths(pts, nrm, samples=K, ray_eps=G.EPS, max_depth=8, rr_start=3)
    assert not same(pE, E) and pst.rays == ref.segments


def test_other_state_is_untouched(P, pto, glass):
    """9. A PT_FLAG_ACCUMULATE sequence with a flagged pt_gather_paths in the middle is the sequence without it, and the framebuffer, the
    denoised and displayed images, the guides and the temporal history of the frame survive the call (gather_device's sequence, with
    the flagged call)."""
    N = P.native
    sd, pts, nrm, _ = glass
    rec = G.records(pts, nrm)

    def sequence(with_gather):
        r = P.Renderer(P.Window(G.W, G.H))
        r.Init()
        try:
            r.SetScene(sd, 0)
            r.Params = P.make_params(G.W, G.H, spp=2, max_depth=4, streams=2)
            r.Render(0.0)
            r.Denoise()
            r.DenoiseTemporal()
            r.Display()
            kept = lambda: (r.ReadFramebuffer(), r.ReadDenoised(), r.ReadDisplay().astype(np.float32), r.ReadTemporal(), r.ReadGuides(),
                            r.ReadHistoryLength())
            before = kept()
            if with_gather:
                out, st = GN.call(P, r, rec, ray_eps=G.EPS)
                assert out[:, 3].min() >= 0 and st.rays > K * len(rec)
                changed = [j for j, (a, b) in enumerate(zip(kept(), before)) if not same(np.asarray(a, np.float32), np.asarray(b, np.float32))]
                assert not changed, ("the call changed (0 framebuffer, 1 denoised, 2 display, 3 temporal, 4 guides, 5 history length)", changed)
            r.Params = P.make_params(G.W, G.H, spp=2, max_depth=4, streams=2, sample_offset=2, flags=N.PT_FLAG_ACCUMULATE)
            st = r.Render(0.0)
            return r.ReadFramebuffer(), int(st.rays)
        finally:
            r.Dispose()

    a, b = sequence(True), sequence(False)
    assert same(a[0], b[0]) and a[1] == b[1], ("the accumulated frame differs", int((bits(a[0]) != bits(b[0])).sum()), a[1], b[1])
