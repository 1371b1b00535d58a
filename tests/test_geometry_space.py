"""The oracle's closest hit against the float64 caster across the geometry space (tests/geometry_space.py): translated, rescaled,
stretched, flat, nested and degenerate scenes, needles, and cameras and spheres far away. Brute force and the host builder's blob for
every layout. A disagreement must be an edge, two surfaces at one distance or, for a sphere far away in its own radii, inside the
band SPEC §4's cancelling discriminant leaves uncertain (ray_caster64.K_S); anything else fails. The device's side of this is
tests/test_gpu_geometry_space.py."""
import numpy as np
import pytest

import geometry_space as G
import ray_caster64 as rc
from float64_support import build_bvh_detached
from geometry_space import CASE_NAMES, COUNTS, case_ray_sets, cases, check_case
from trace_support import LAYOUTS, oracle, ray_sets


@pytest.mark.parametrize("name", CASE_NAMES)
def test_oracle_matches_float64_across_the_geometry_space(P, pto, name):
    """Every in-domain case: brute force and the host builder's blob of every layout (which validates) against the caster."""
    case = cases()[name]
    assert case.in_domain
    sd = case.sd
    scenes = [("brute", pto.Scene(sd))]
    for layout in LAYOUTS:
        info, nodes, tris = build_bvh_detached(sd, layout)
        osc = pto.Scene(sd, (info.width, nodes, tris))
        assert osc.validate_bvh()[0] == 0, (name, layout)
        scenes.append((layout, osc))
    for rs, o, d in case_ray_sets(pto, case):
        cast = rc.cast(sd.verts, sd.spheres, o, d)
        first = None
        for layout, osc in scenes:
            ids, _, _ = oracle(pto, osc, o, d)
            if first is None:
                first = ids
                check_case(case, rs, o, d, ids, cast, (name, rs, layout))
            elif not np.array_equal(ids, first):  # (equal ids classify equally)
                check_case(case, rs, o, d, ids, cast, (name, rs, layout))


def test_case_list_is_the_in_domain_set():
    assert sorted(CASE_NAMES) == sorted(c.name for c in G.in_domain_cases())
    assert [c.name for c in G.out_of_domain()] == ["scale_glass_-50", "scale_glass_+44", "scale_tess_-50", "scale_tess_+44"]


def test_out_of_domain_scales_lose_hits(P, pto):
    """The first exponents outside the closest hit's envelope: the id image of the glass box differs from float64 (which is why they
    are outside), on brute force as on a blob."""
    for name in ("scale_glass_-50", "scale_glass_+44"):
        case = cases()[name]
        o, d = G.case_rays(pto, case)
        ids, _, _ = oracle(pto, pto.Scene(case.sd), o, d)
        assert len(rc.classify(case.sd.verts, case.sd.spheres, o, d, ids)["wrong"]) > 0, name


def _sphere_f32(o, d, c, r):
    """SPEC §4's sphere test restated in numpy float32, one sphere: ids (0 or MISS). The fma is taken in float64, where b*b is exact."""
    f = np.float32
    oc = o - c.astype(f)
    dot = lambda a, b: (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]  # noqa: E731
    b = dot(oc, d)
    cc = dot(oc, oc) - f(r) * f(r)
    disc = (b.astype(np.float64) * b.astype(np.float64) - cc.astype(np.float64)).astype(f)
    with np.errstate(invalid="ignore"):
        s = np.sqrt(disc)
        t0, t1 = -b - s, -b + s
        t = np.where(t0 > 0, t0, t1)
        hit = (disc > 0) & (t > 0)
    return np.where(hit, 0, rc.MISS).astype(np.uint64)


def test_radius_control(P, pto):
    """The checker sees a sphere test whose radius is off, at 100 radii, on rays around the silhouette. A ring at 1.0005 r: the true
    restatement (which equals the oracle on the fan, ray by ray) misses as float64 does, a radius of 1.001 r hits and is `wrong` under
    the default band. The scaled band is 0.46 % of r² at 100 radii, wider than the 0.2 % by which 0.1 % of radius moves the
    discriminant, so under it the same control takes a ring at 1.005 r and a radius of 1.01 r."""
    case = cases()["far_sphere_100"]
    sph = case.sd.spheres
    o, d = case.rays
    assert np.array_equal(_sphere_f32(o, d, sph[0, :3], sph[0, 3]), np.where(oracle(pto, pto.Scene(case.sd), o, d)[0] == rc.MISS, rc.MISS, 0))
    for ring, radius, kw in ((1.0005, 1.001, {}), (1.005, 1.01, dict(sphere_band=True))):
        o, d = G.silhouette_ring(case, ring)
        wrong = lambda r: len(rc.classify(case.sd.verts, sph, o, d, _sphere_f32(o, d, sph[0, :3], np.float32(r) * sph[0, 3]), **kw)["wrong"])  # noqa: E731
        assert wrong(1.0) == 0 and wrong(radius) > 0, (ring, wrong(1.0), wrong(radius))


def test_default_band_control(P, pto):
    """The cases reach the cancellation: without the scaled band, far_sphere at 1000 radii has `wrong` rays."""
    case = cases()["far_sphere_1000"]
    o, d = case.rays
    ids, _, _ = oracle(pto, pto.Scene(case.sd), o, d)
    assert len(rc.classify(case.sd.verts, case.sd.spheres, o, d, ids)["wrong"]) > 0
    assert len(rc.classify(case.sd.verts, case.sd.spheres, o, d, ids, sphere_band=True)["wrong"]) == 0


def test_bands_are_arguments(P, pto):
    """Per-ray bands: the default values as arrays classify as the defaults do; a zero edge band turns edge rays into wrong ones."""
    case = cases()["translate_tess_3"]
    o, d = G.case_rays(pto, case)
    rng = np.random.default_rng(1)
    ids, _, _ = oracle(pto, pto.Scene(case.sd), o, d)
    ids[rng.integers(0, len(ids), 40)] = rc.MISS  # some real disagreements
    cast = rc.cast(case.sd.verts, case.sd.spheres, o, d)
    a = rc.classify(case.sd.verts, case.sd.spheres, o, d, ids, cast)
    b = rc.classify(case.sd.verts, case.sd.spheres, o, d, ids, cast, edge_band=np.full(len(o), rc.EDGE_BAND), t_band=np.full(len(o), rc.T_BAND))
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert len(a["wrong"]) > 0 and len(a["coincident"]) > 0
    z = rc.classify(case.sd.verts, case.sd.spheres, o, d, ids, cast, edge_band=0.0, t_band=0.0)
    assert len(z["edge"]) == 0 and len(z["coincident"]) < len(a["coincident"])  # (candidates with the very same t stay)
    assert len(z["wrong"]) + len(z["coincident"]) == len(a["wrong"]) + len(a["edge"]) + len(a["coincident"])


def test_origin_class_is_not_vacuous(P, pto):
    """On the rays the `origin` class excuses, only the two ids in question pass: with any other id in their place they are `wrong`;
    and without the floor they are `wrong` as they stand."""
    case = cases()["needles_0.0001"]
    sd = case.sd
    _, o, d = [s for s in ray_sets(pto, sd, n=G.N_RAYS) if s[0] == "on_surface"][0]
    ids, _, _ = oracle(pto, pto.Scene(sd), o, d)
    cast = rc.cast(sd.verts, sd.spheres, o, d)
    floor = 16 * np.spacing(np.abs(o).max(axis=1)).astype(np.float64)
    c = rc.classify(sd.verts, sd.spheres, o, d, ids, cast, t_floor=floor)
    rays = c["origin"]
    assert len(rays) > 5 and len(c["wrong"]) == 0
    assert set(rays) <= set(rc.classify(sd.verts, sd.spheres, o, d, ids, cast)["wrong"])
    small = len(sd.tri_mat) + 3  # the smallest sphere, which none of these rays meets; nor does any leave the closed box
    assert not np.isin([rc.MISS, small], np.concatenate([ids[rays], c["want"][rays]])).any()
    for other in (rc.MISS, small):
        bad = ids.copy()
        bad[rays] = other
        assert set(rays) <= set(rc.classify(sd.verts, sd.spheres, o, d, bad, cast, t_floor=floor)["wrong"]), other


def test_k_s_is_twice_the_measured_value(P, pto):
    """The measurement behind ray_caster64.K_S, repeated: over far_sphere and far_camera, on brute force, the largest
    |disc64|/r² / ((|oc|/r)² · 2^-24) among the rays where the oracle disagrees with float64 is K_S_MEASURED (below 8: rounding alone)."""
    worst = 0.0
    for case in cases().values():
        if case.family not in ("far_sphere", "far_camera") or not case.sphere_band:
            continue
        o, d = G.case_rays(pto, case)
        ids, _, _ = oracle(pto, pto.Scene(case.sd), o, d)
        c = rc.classify(case.sd.verts, case.sd.spheres, o, d, ids, sphere_band=True)
        r = c["sphere_ratio"][ids != c["want"]]
        worst = max([worst] + list(r[np.isfinite(r)]))
    COUNTS["K_S measured"] = worst
    assert worst < 8 and rc.K_S_MEASURED - 0.01 <= worst <= rc.K_S_MEASURED and rc.K_S == 2 * rc.K_S_MEASURED
