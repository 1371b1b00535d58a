"""-m gpu: pt_gather_paths with PT_GATHER_PATHS_NEXT_EVENT | PT_GATHER_PATHS_SPHERE_LIGHTS (include/ptrt.h, docs/SPEC.md §7.1 in §12.2) against
the scalar checker of tests/gather_sphere_ref/.

Every comparison is bit for bit — the eight floats of every record and pt_stats::rays (segments + shadow rays). The points are 200 of the
first hits of a 24 x 18 camera frame (gather_ref.first_hits) — not a multiple of 64 — with K = 16 and ray_eps = 1e-3 unless a test says
otherwise. Every test commits its own scene on the session's renderer."""
import dataclasses

import numpy as np
import pytest

import gather_nee_checker as GN
import gather_ref as G
import gather_sphere_checker as GS
import nee_checker as nc
import sphere_light_checker as sc
from gather_device import LBVH, SENTINEL, bits, same

pytestmark = pytest.mark.gpu
N_POINTS, K = 200, 16


def held(P, r, osc, pts, nrm, ctx, env=None, host=True, ref=None, **kw):
    """One flagged call on the device and the checker's: the same bits, the same rays."""
    kw = {"ray_eps": G.EPS, "samples": K, **kw}
    out, st = GS.call(P, r, G.records(pts, nrm), host=host, **kw)
    ref = ref or GS.gather(osc, pts, nrm, env=env, **kw)
    bad = np.nonzero((bits(out) != bits(ref.rows)).any(1))[0]
    assert len(bad) == 0, (ctx, len(bad), bad[:4], out[bad[:2]], ref.rows[bad[:2]])
    assert st.rays == ref.rays and st.paths == len(pts), (ctx, st.rays, ref.segments, ref.shadow_rays)
    assert np.isfinite(out).all()
    return out, st, ref


def _case(P, pto, name):
    sd = sc.scene(P, name, G.W, G.H)
    pts, nrm = G.first_hits(P, pto, sd)
    assert len(pts) >= N_POINTS
    sel = np.linspace(0, len(pts) - 1, N_POINTS).astype(int)
    osc = pto.Scene(sd)
    osc.build_own_bvh()
    return sd, pts[sel], nrm[sel], osc


@pytest.fixture(scope="module")
def cases(P, pto):
    return {name: _case(P, pto, name) for name in ("lamp", "lamp+quad", "glass-lamp")}


def test_layouts_maps_and_depths(P, pto, renderer, cases):
    """13. Every layout (and the GPU builder), with and without a lit map, max_depth 1 and 8, lit by a lamp only, by the lamp and the quad,
    and by an emissive glass ball: the checker's bits and rays, and so the same on every layout."""
    env = sc.lit_map(P, 8)
    for name, (sd, pts, nrm, osc) in cases.items():
        for e in (None, env):
            first, refs = {}, {}
            for width in (2, 4, 68, 72, 73, 68 | LBVH):
                renderer.SetScene(sd if e is None else dataclasses.replace(sd, environment=e), width)
                for md, rr in ((8, 3), (1, 0)):
                    out, st, refs[md] = held(P, renderer, osc, pts, nrm, (name, e is not None, width, md), env=e, ref=refs.get(md), max_depth=md,
                                             rr_start=rr)
                    assert refs[md].n_sphere_lights == 1 and refs[md].shadow_rays > 0 and refs[md].lit == (e is not None)
                    assert same(out, first.setdefault(md, out)), ("layouts differ", name, width, md)


def test_split_calls_visibility_and_sentinel(P, pto, renderer, cases):
    """13. A bake split by point_offset (the cut inside a wave) and by sample_offset is the checker's for the same offsets, and the point
    split is the unsplit bake; visibility and bent are pt_gather_paths's bits without the flags, for an unbounded and a bounded
    max_distance, and rays(flagged) - rays(unflagged) is the checker's shadow-ray count; an invalid point gets its sentinel record; the
    device-memory path gives the same bits."""
    sd, pts, nrm, osc = cases["lamp+quad"]
    rec = G.records(pts, nrm)
    renderer.SetScene(sd, 0)
    whole, st, ref = held(P, renderer, osc, pts, nrm, "whole")
    h = N_POINTS // 2 + 1
    assert h % 4 != 0
    a, sa, _ = held(P, renderer, osc, pts[:h], nrm[:h], "first half")
    b, sb, _ = held(P, renderer, osc, pts[h:], nrm[h:], "second half", point_offset=h)
    assert same(np.concatenate([a, b]), whole) and sa.rays + sb.rays == st.rays
    held(P, renderer, osc, pts, nrm, "later samples", sample_offset=K)
    dev, _, _ = held(P, renderer, osc, pts, nrm, "device memory", host=False, ref=ref)
    assert same(dev, whole)
    for dist in (0.0, G.half_box(sd)):
        f, sf = GS.call(P, renderer, rec, samples=K, max_distance=dist, ray_eps=G.EPS)
        u, su = GS.call(P, renderer, rec, samples=K, next_event=False, sphere_lights=False, max_distance=dist, ray_eps=G.EPS)
        assert same(f[:, 3:], u[:, 3:]) and same(f[:, :3], whole[:, :3]), dist  # shadow rays and paths ignore max_distance
        assert sf.rays - su.rays == ref.shadow_rays and su.rays == ref.segments
    bad = rec.copy()
    bad[3, 4:7] = 0.0       # no normal
    bad[77, 0] = np.nan     # no position
    out, sbad = GS.call(P, renderer, bad, samples=K, ray_eps=G.EPS)
    assert same(out[[3, 77]], np.tile(SENTINEL, (2, 1))) and same(np.delete(out, [3, 77], 0), np.delete(whole, [3, 77], 0))


def test_without_a_sphere_light_and_without_the_flag(P, pto, renderer, cases):
    """11. / 13. On a scene without a sphere light the flagged call is the PT_GATHER_PATHS_NEXT_EVENT call bit for bit, rays included; on
    a scene with one, the call without the new flag is still gather_nee_checker's."""
    for sd in (G.scene(P, "glass"), sc.without_sphere_emission(nc.many_lights_scene(P, G.W, G.H))):
        pts, nrm = G.first_hits(P, pto, sd)
        rec = G.records(pts[:N_POINTS], nrm[:N_POINTS])
        renderer.SetScene(sd, 0)
        a, sa = GS.call(P, renderer, rec, samples=K, ray_eps=G.EPS)
        b, sb = GS.call(P, renderer, rec, samples=K, sphere_lights=False, ray_eps=G.EPS)
        assert same(a, b) and sa.rays == sb.rays
    sd, pts, nrm, osc = cases["lamp+quad"]
    renderer.SetScene(sd, 0)
    out, st = GS.call(P, renderer, G.records(pts, nrm), samples=K, sphere_lights=False, ray_eps=G.EPS)
    ref = GN.gather(osc, pts, nrm, samples=K, ray_eps=G.EPS)
    assert same(out, ref.rows) and st.rays == ref.rays


def test_a_moved_lamp_is_sampled_where_it_is(P, pto, renderer, cases):
    """10. After pt_scene_update_spheres moves and resizes the lamp the flagged gather equals the checker's on the updated scene."""
    sd, pts, nrm, _ = cases["lamp"]
    sph = sd.spheres.copy()
    sph[-1] = (0.4, 0.2, -0.3, 0.25)
    moved = dataclasses.replace(sd, spheres=sph)
    osc = pto.Scene(moved)
    renderer.SetScene(sd, 0)
    renderer.UpdateGeometry(spheres=sph)
    held(P, renderer, osc, pts, nrm, "moved lamp")


def test_refusals(P, renderer, cases):
    """12. The sphere bit without the NEE bit, and bit 8, are PT_ERR_INVALID_ARGUMENT on a live context too, and the next call is right."""
    import ctypes as C
    N = P.native
    sd, pts, nrm, osc = cases["lamp"]
    renderer.SetScene(sd, 0)
    rec = G.records(pts, nrm)
    out = np.zeros_like(rec)
    gp = N.pt_gather_params(samples=K, ray_eps=G.EPS, flags=N.PT_GATHER_HOST_MEMORY)
    for flags, text in ((16, b"needs PT_GATHER_PATHS_NEXT_EVENT"), (4 | 8, b"unknown path flag"), (4 | 16 | 8, b"unknown path flag")):
        pp = N.pt_gather_path_params(max_depth=8, rr_start=3, flags=flags)
        rc = N.lib.pt_gather_paths(renderer._ctx, renderer._scene, rec.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), len(rec),
                                   C.byref(gp), C.byref(pp), None)
        assert rc == N.PT_ERR_INVALID_ARGUMENT and text in N.lib.pt_last_error(renderer._ctx), flags
    assert (out == 0).all()
    held(P, renderer, osc, pts, nrm, "after refusals")
