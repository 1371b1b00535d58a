"""-m gpu: the device's closest hit across the geometry space (tests/geometry_space.py), against the oracle bit for bit on the same
blob and against the float64 caster with the caps of tests/test_geometry_space.py.

What the device could get wrong here where the scenes around the origin could not: Morton normalisation and the SAH top storey with
large offsets and flat or stretched bounds (lbvh.hip), the quantiser's grid regrowing in a refit (refit.hip), octant ordering of
layout 73 on flat axes, safe_inv with zero direction components at large |o|, the overflow stack on needle trees, and denormal
products at 2^-40 in the triangle test (the kernels are built not to flush them)."""
import numpy as np
import pytest

import adversarial_scenes as S
import geometry_space as G
import ray_caster64 as rc
from frame_checks import _config_grid, run_both
from geometry_space import CASE_NAMES, PATH_TRACE, case_ray_sets, cases, check_case
from trace_support import LAYOUTS, MISS, check_closest, commit, ids_of, oracle, records, same

pytestmark = pytest.mark.gpu

OUT_OF_DOMAIN = ["scale_glass_-50", "scale_glass_+44", "scale_tess_-50", "scale_tess_+44"]
ID_IMAGE = [n for n in CASE_NAMES if n.split("_")[0] in ("translate", "scale") or n.startswith("far_camera")]


def trace_and_check(pto, renderer, osc, case, sets, ctx, seen):
    """One committed blob: the device's closest hits, visit counters, plain kernel and occlusion against pto_closest on `osc`; in
    the domain, the device's ids against the caster (once per distinct id array: equal ids classify equally)."""
    for rs, o, d, cast in sets:
        ids, ts, ost = oracle(pto, osc, o, d)
        rec = records(o, d)
        hits, st = renderer.TraceRays(rec, count_visits=True)
        check_closest(hits, ids, ts, ctx + (rs,))
        assert st.rays == len(o)
        assert (st.node_visits, st.tri_tests, st.sphere_tests) == (ost.node_visits, ost.tri_tests, ost.sphere_tests), ctx + (rs,)
        assert same(renderer.TraceRays(rec)[0], hits), ctx + (rs,)
        occ, _ = renderer.TraceRays(rec, occlusion=True)
        assert np.array_equal(ids_of(occ) != MISS, ids != MISS), ctx + (rs,)
        got = ids_of(hits)
        if case.in_domain and not any(np.array_equal(got, s) for s in seen.setdefault(rs, [])):
            seen[rs].append(got)
            check_case(case, rs, o, d, got, cast, ctx + (rs, "device"))


@pytest.mark.parametrize("name", CASE_NAMES + OUT_OF_DOMAIN)
def test_trace_matches_oracle_and_float64(P, pto, renderer, name):
    """Every case, in the domain and just outside it (where the answer is wrong but specified), every layout, both builders."""
    case = cases()[name]
    sets = [(rs, o, d, rc.cast(case.sd.verts, case.sd.spheres, o, d) if case.in_domain else None) for rs, o, d in case_ray_sets(pto, case)]
    seen = {}
    for width in LAYOUTS:
        for build in (0, P.native.PT_BVH_BUILD_LBVH):
            osc = commit(P, pto, renderer, case.sd, width | build)
            trace_and_check(pto, renderer, osc, case, sets, (name, width, build), seen)


@pytest.mark.parametrize("name", ID_IMAGE)
def test_id_image_matches_the_query(P, pto, renderer, name):
    """pt_render's primary hits of the unjittered camera rays: the id image equals the oracle's on the same blob and the ids
    pt_trace_rays returns for those rays, for every layout with the builders alternating."""
    case = cases()[name]
    ids = S.id_scene(case.sd)
    o, d = rc.camera_rays(pto, ids.cam, G.W, G.H)
    for i, width in enumerate(LAYOUTS):
        build = P.native.PT_BVH_BUILD_LBVH if i % 2 else 0
        img, st, ref, ost = run_both(P, pto, renderer, ids, S.params_id(G.W, G.H, ray_eps=case.ray_eps), width | build)
        assert st.rays == ost.rays == G.W * G.H and np.array_equal(img, ref), (name, width, build)
        hits, _ = renderer.TraceRays((o, d))
        assert np.array_equal(ids_of(hits), S.ids_of(img)), (name, width, build)


@pytest.mark.parametrize("name", PATH_TRACE)
def test_full_path_trace(P, pto, renderer, name):
    """47 x 35, spp 3, depth 8, two streams, the case's ray_eps, on the twelve configurations of frame_checks._config_grid
    (every extend kernel counting and plain, the layouts and builders cycling): frame, rays, paths and visit counters are the
    oracle's, and Render raises nothing (BvhInfo().stack_need is reachable: a stack overflow raises). The needle case's trees need
    more than the 12 LDS entries, so its rays run through the overflow columns."""
    case = cases()[name]
    for width, flags, count in _config_grid(P):
        p = P.make_params(47, 35, spp=3, max_depth=8, streams=2, flags=flags, ray_eps=case.ray_eps)
        img, st, ref, ost = run_both(P, pto, renderer, case.sd, p, width, count=count)
        ctx = (name, width, flags, count)
        assert st.rays == ost.rays and st.paths == ost.paths and np.array_equal(img, ref), ctx
        if count:
            assert (st.node_visits, st.tri_tests, st.sphere_tests) == (ost.node_visits, ost.tri_tests, ost.sphere_tests), ctx
        if case.family == "needles":
            assert renderer.BvhInfo().stack_need > 12, ctx


def _placements(pto):
    """(the committed box, [(pseudo case of the moved scene, its camera rays)]) for the refit: geometry_space.refit_cases."""
    base, out = G.refit_cases()
    return base, [(c, G.case_rays(pto, c)) for c in out]


@pytest.mark.parametrize("width", [68, 2 | 0x100])
def test_refit_across_the_geometry_space(P, pto, renderer, width):
    """The tessellated box committed at the origin, then moved by UpdateGeometry to each placement, fed once from a numpy array and
    once from a torch device tensor: the refitted blob validates, traces equal the oracle on it and pass the caster's classification,
    both feeds give the same hits, and updating back restores the original hits bit for bit."""
    import torch
    assert 0x100 == P.native.PT_BVH_BUILD_LBVH
    base, placements = _placements(pto)
    renderer.SetScene(base, width)
    o0, d0 = rc.camera_rays(pto, base.cam, G.W, G.H)
    hits0, _ = renderer.TraceRays((o0, d0))
    assert (ids_of(hits0) != MISS).sum() == 1190
    for case, (o, d) in placements:
        sd = case.sd
        cast = rc.cast(sd.verts, sd.spheres, o, d)
        first = None
        for feed in ("numpy", "torch"):
            verts = torch.from_numpy(np.ascontiguousarray(sd.verts, np.float32)).cuda() if feed == "torch" else sd.verts
            renderer.UpdateGeometry(verts=verts, spheres=sd.spheres)
            info = renderer.BvhInfo()
            osc = pto.Scene(sd, (info.width,) + renderer.BvhRead())
            assert osc.validate_bvh()[0] == 0, (case.name, width, feed)
            if first is None:
                trace_and_check(pto, renderer, osc, case, [("camera", o, d, cast)], (case.name, width, feed), {})
                first = renderer.TraceRays((o, d))[0]
            else:
                assert same(renderer.TraceRays((o, d))[0], first), (case.name, width, feed)
            renderer.UpdateGeometry(verts=base.verts, spheres=base.spheres)
            assert same(renderer.TraceRays((o0, d0))[0], hits0), (case.name, width, feed)
