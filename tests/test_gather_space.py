"""CPU checks of what tests/test_gpu_gather_space.py trusts: the scalar checker of tests/gather_paths_ref/ held to the Python restatement
of §12 (tests/gather_ref.py), and that restatement to the float64 ray caster, on the inputs of the gather tests across the geometry space
(gather_ref.space_case): the probe set of the stacked layers, a translated, a needle and a scaled case of tests/geometry_space.py and the
64-sphere list. At most 64 points (gather_ref.spread) x 16 samples per case: the Python ray loop is the slow part.

A case runs with its own ray_eps (geometry_space.Case.ray_eps). For translate_glass_2 that is 1e-4 * 65537 = 6.55 on a box two units
across: every origin lies outside the box and every ray leaves (1024 of 1024 visible). That is what the case's path trace uses, and
the gathers are held to it; but on-surface origins at large coordinates are only reached with a ray_eps next to the coordinates' ulp,
so the case also runs with gather_ref.tight_eps (32 ulps of 65537 = 0.25), named translate_glass_2/tight here.

Measured shares of clear rays (gather_ref.clear_rays: not near an edge of the hit, not in a triangle's plane, the hit not near
max_distance), unbounded / with max_distance about half the extent, and visible samples of the 1024 unbounded:
  layers                 1.000 / 1.000   163 visible
  translate_glass_2      1.000 / 1.000   1024 visible (see above)
  translate_glass_2/tight 1.000 / 1.000  264 visible
  needles_0.0001         1.000 / 1.000   237 visible
  scale_glass_+40        1.000 / 1.000   238 visible
  spheres64              1.000 / 1.000   552 visible
No case fell below the 0.8 of tests/test_gather.py; none was swapped."""
import dataclasses

import numpy as np
import pytest

import gather_paths_checker as GP
import gather_ref as G
import ray_caster64 as rc
from float64_support import build_bvh_detached
from trace_support import LAYOUTS

SKY = np.array([1.0, 2.0, 3.0], np.float32)
SAMPLES = 16
CASES = ["layers", "translate_glass_2", "translate_glass_2/tight", "needles_0.0001", "scale_glass_+40", "spheres64"]
_RAYS = {}


def inputs(P, pto, name):
    """(scene, at most 64 points, normals, ray_eps, oracle scene without emission under SKY, gather_ref.Rays with 16 samples), once."""
    if name not in _RAYS:
        base, _, tight = name.partition("/")
        sd, pts, nrm, eps = G.space_case(P, pto, base)
        if tight:
            eps = G.tight_eps(sd)
        pts, nrm = G.spread(pts, nrm)
        assert 32 <= len(pts) <= 64, (name, len(pts))
        osc = pto.Scene(dataclasses.replace(GP.without_emission(sd), sky=SKY))
        osc.build_own_bvh()
        _RAYS[name] = (sd, pts, nrm, eps, osc, G.rays(P, pto, osc, pts, nrm, SAMPLES, ray_eps=eps))
    return _RAYS[name]


def test_probe_rays_overflow_the_lds_stack(P, pto):
    """The sample rays of the probe set on the stacked layers, walked through the product's blob in float64 (ray_caster64.stack_depth):
    on every layout the tree needs more than the 12 LDS entries and some ray of the set holds more than 12 (measured: at least 97 % of
    them, up to stack_need itself), so a gather of the set runs through the overflow columns."""
    sd, pts, nrm, eps, _, rays = inputs(P, pto, "layers")
    assert len(pts) == 64 and rays.valid.all()
    for layout in LAYOUTS:
        info, nodes, tris = build_bvh_detached(sd, layout)
        assert info.stack_need > 12, (layout, info.stack_need)
        depth = [rc.stack_depth(layout, nodes, tris, rays.o[i], rays.d[i, k]) for i in range(0, len(pts), 7) for k in range(0, SAMPLES, 5)]
        assert max(depth) > 12, (layout, max(depth))
        assert max(depth) <= info.stack_need, (layout, max(depth), info.stack_need)


@pytest.mark.parametrize("name", CASES)
def test_checker_is_the_sky_gather(P, pto, name):
    """B1. The checker with max_depth 1 on the scene without emitters is §12 as gather_ref states it: the counts exactly, bent within
    (K + 2) 2^-24 and E within that of sum |term| / K (tests/test_gpu_gather.py derives the bound), unbounded and with max_distance
    about half the extent; one segment per sample."""
    sd, pts, nrm, eps, osc, rays = inputs(P, pto, name)
    b = (SAMPLES + 2) * 2.0 ** -24
    for md in (0.0, G.half_box(sd)):
        ref = G.gather(rays, md, sky=SKY)
        r = GP.gather(osc, pts, nrm, samples=SAMPLES, max_distance=md, ray_eps=eps, max_depth=1, rr_start=0)
        assert r.rays == SAMPLES * len(pts), (name, md)
        assert np.array_equal(np.rint(r.visibility.astype(np.float64) * SAMPLES).astype(np.int64), ref["count"]), (name, md)
        assert (np.abs(r.bent.astype(np.float64) - ref["bent"]) <= b).all(), (name, md)
        if md == 0.0:  # (with a finite max_distance §12's E also takes the sky behind an occluder farther than that; a path does not)
            assert (np.abs(r.E.astype(np.float64) - ref["E"]) <= b * ref["absE"]).all(), name
    whole = G.gather(rays, 0.0, sky=SKY)["count"].sum()
    assert whole > 0 and (whole < SAMPLES * len(pts) or name == "translate_glass_2"), (name, whole)  # (the module's docstring)


@pytest.mark.parametrize("name", CASES)
def test_reference_agrees_with_float64(P, pto, name):
    """B2. gather_ref's visibility of every ray equals the float64 caster's occlusion on the rays that are clear, and more than 0.8 of
    the rays are clear (the rule of tests/test_gather.py), unbounded and with max_distance about half the extent."""
    sd, pts, nrm, eps, _, rays = inputs(P, pto, name)
    assert rays.valid.all() and np.abs(np.linalg.norm(rays.d.astype(np.float64), axis=2) - 1).max() < 1e-6
    cast = G.cast_rays(sd, rays)
    for md in (0.0, G.half_box(sd)):
        occluded, clear = G.clear_rays(rays, cast, md)
        V = G.visible(rays, md)
        print(f"{name}: max_distance {md:g}: clear {clear.mean():.4f}, visible {int(V.sum())} of {V.size}")
        assert clear.sum() > 0.8 * clear.size, (name, md, clear.mean())
        assert np.array_equal(V[clear], ~occluded[clear]), (name, md, np.argwhere(clear & (V == occluded))[:8])


def test_the_points_distinguish(P, pto):
    """B3. On translate_glass_2 the checker with one of its deliberate errors (the throughput without W) and the checker with ray_eps = 0
    each give other bits than the checker: with the tight ray_eps, where the paths bounce inside the box, for both; with the case's own
    ray_eps, at which every path leaves with its first segment and no throughput is ever used, for ray_eps = 0."""
    sd, pts, nrm, own = G.space_case(P, pto, "translate_glass_2")
    osc = pto.Scene(sd)
    osc.build_own_bvh()
    same = lambda a, b: np.array_equal(a.rows.view(np.uint32), b.rows.view(np.uint32)) and a.rays == b.rays
    for eps in (G.tight_eps(sd), own):
        good = GP.gather(osc, pts, nrm, ray_eps=eps)
        assert same(good, GP.gather(osc, pts, nrm, ray_eps=eps))
        assert not same(good, GP.gather(osc, pts, nrm, ray_eps=0.0)), eps
        if eps != own:
            assert good.rays > G.K * len(pts)
            assert not same(good, GP.gather(osc, pts, nrm, ray_eps=eps, flags=GP.NO_W))
        else:
            assert good.rays == G.K * len(pts)
