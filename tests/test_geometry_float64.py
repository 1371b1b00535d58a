"""The oracle's closest hit against a float64 ray caster (tests/ray_caster64.py) on adversarial scenes, and the properties of
those scenes the GPU tests rely on. The oracle restates the f32 spec; the caster answers the geometric question, so these
pin the spec's geometry itself. A disagreement must be explained by an edge (within EDGE_BAND, a miss there is a crack) or by
two surfaces at the same distance; anything else fails."""
import numpy as np
import pytest

import adversarial_scenes as S
import ray_caster64 as rc
import geometry_space as G
from float64_support import H, PINNED_CRACKS, W, _size, build_bvh_detached, check_classes, crack_rays, oracle_ids, scenes
from geometry_space import SCALE_FIRST_BAD, SCALE_K
from trace_support import LAYOUTS, oracle


@pytest.mark.parametrize("layout", LAYOUTS)
def test_oracle_closest_hit_matches_float64(P, pto, layout):
    """Every adversarial scene: the oracle's primary-hit id image (pto_render of an id_scene) classified against the caster.
    The floor camera's centre row lies in the floor's plane; those rays are the only ones left out."""
    for name, sd in scenes(P).items():
        w, h = _size(name)
        o, d = rc.camera_rays(pto, S.id_scene(sd).cam, w, h)
        c = check_classes(sd, o, d, oracle_ids(pto, sd, layout, w, h), name)
        if name == "floor":
            assert list(c["in_plane"]) == [(h // 2) * w + x for x in range(w)]
        else:
            assert len(c["in_plane"]) == 0, name
        if name in ("duplicates", "layers", "inside_sphere"):
            assert len(c["edge"]) + len(c["coincident"]) <= 8, name


def test_pto_closest_matches_float64(P, pto):
    """pto.closest on single rays (brute force and the product's blob) agrees with the caster on the duplicates scene: the lowest
    id of a tie wins, whichever leaf it sits in."""
    sd, src = S.duplicates(W, H)
    o, d = rc.camera_rays(pto, S.id_scene(sd).cam, W, H)
    sel = np.arange(0, len(o), 7)
    info, nodes, tris = build_bvh_detached(sd, 68)
    for sc in (pto.Scene(sd), pto.Scene(sd, (info.width, nodes, tris))):
        ids = np.array([sc.closest(o[i], d[i])[0] for i in sel], np.uint64)
        c = check_classes(sd, o[sel], d[sel], ids, "duplicates")
        hit = ids != rc.MISS
        assert hit.sum() > 0.6 * len(sel)
        # the winner is the lowest id among the copies of its source triangle
        for i in np.nonzero(hit & (ids < len(src)))[0]:
            assert ids[i] == np.nonzero(src == src[ids[i]])[0].min()
        assert np.array_equal(ids[hit], c["want"][hit])


def test_camera_ray_binding(P, pto):
    """pto.camera_ray is SPEC §3: the axis camera's centre row and column have direction components of exactly zero."""
    sd = S.axis_camera(P.make_scene(0, 0, 1, W, H), W, H)
    o, d = pto.camera_ray(sd.cam, W // 2, H // 2)
    assert o.dtype == np.float32 and list(d) == [0.0, 0.0, -1.0]
    assert pto.camera_ray(sd.cam, 3, H // 2)[1][1] == 0.0 and pto.camera_ray(sd.cam, W // 2, 5)[1][0] == 0.0
    _, d = pto.camera_ray(S.ray_camera(sd, (0, 0, 0), (3, 0, -4)).cam, 0, 0)
    assert np.allclose(d, [0.6, 0, -0.8], atol=1e-7)


def test_caster_in_plane_rule():
    """A ray is left out as in-plane only if it touches a triangle whose plane it lies in: not for a coplanar triangle off to
    the side, nor for one behind its origin."""
    verts = np.float32([[0, 0, -1, 1, 0, -1, 0, 0, -2],        # all in the plane y = 0
                        [5, 0, -1, 6, 0, -1, 5, 0, -2],
                        [0, 0, 1, 1, 0, 1, 0, 0, 2]])
    o = np.float32([[0.2, 0, 0], [0.2, 0, -1.2], [0.2, 0, 0], [0.2, 0, 3]])
    d = np.float32([[0, 0, -1], [1, 0, 0], [0, 0, 1], [0, 0, 1]])
    # ray 0 runs across triangle 0; ray 1 starts inside triangle 0 and crosses triangle 1; ray 2 crosses triangle 2;
    # ray 3 has every triangle behind it
    no_spheres = np.zeros((0, 4), np.float32)
    assert list(rc.cast(verts, no_spheres, o, d)[3]) == [True, True, True, False]
    for tri, want in ((0, [True, True, False, False]), (1, [False, True, False, False]), (2, [False, False, True, False])):
        assert list(rc.cast(verts[tri:tri + 1], no_spheres, o, d)[3]) == want, tri
    # triangles without area (a repeated vertex, collinear vertices with the midpoint in the middle, a point), on or beside the
    # rays: cross(e1, e2) == 0, so every ray has det == 0 and a zero offset from their "plane". They make no ray in-plane, are never
    # hit, and leave the other triangles' answers alone.
    flat = np.float32([[0.2, 0, -1, 0.2, 0, -1, 0.2, 0, -3], [0.2, 0, -1, 0.2, 0, -2, 0.2, 0, -3], [0.2, 0, -1.5] * 3, [7, 7, 7, 7, 7, 7, 8, 9, 10]])
    for k in range(len(flat)):
        assert list(rc.cast(flat[k:k + 1], no_spheres, o, d)[3]) == [False] * 4, k
    assert (rc.cast(flat, no_spheres, o, d)[0] == rc.MISS).all()
    mixed = np.concatenate([flat[:2], verts, flat[2:]])
    ids, _, _, in_plane = rc.cast(mixed, no_spheres, o, d)
    assert list(in_plane) == [True, True, True, False] and not np.isin(ids, [0, 1, 5, 6]).any()
    off = np.float32([[0.2, 1, 0]] * 2)  # off the plane y = 0, aimed at triangle 0 of `verts` through the zero-area ones' line
    ids, _, _, in_plane = rc.cast(mixed, no_spheres, off, np.float32([[0, -0.6, -0.8], [0, -1, -1.5]]))
    assert not in_plane.any() and list(ids) == [2, 2]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_stacked_layers_overflow_the_lds_stack(P, pto, layout):
    """Walking the product's blob (SPEC §4 push order, float64 boxes shrunk by a margin) shows that every sampled camera ray of
    the stacked-layers scene holds more than 12 + 4 stack entries, and never more than pt_bvh_info.stack_need."""
    sd = S.stacked_layers(W, H)
    info, nodes, tris = build_bvh_detached(sd, layout)
    o, d = rc.camera_rays(pto, sd.cam, W, H)
    depth = [rc.stack_depth(layout, nodes, tris, o[i], d[i]) for i in range(0, len(o), 53)]
    assert min(depth) > 12 + 4, (layout, min(depth))
    assert max(depth) <= info.stack_need, (layout, max(depth), info.stack_need)


def test_sphere_list_limit(P):
    """64 spheres are accepted, 65 are refused at the API (kMaxSpheres: they are a flat list)."""
    build_bvh_detached(S.sphere_list(64, 16, 16))
    with pytest.raises(P.PtException):
        build_bvh_detached(S.sphere_list(65, 16, 16))


# SCALE_K, the envelope exponent: the largest |k|, in steps of 2 from 30, at which these frames stay bit-identical and the glass box's
# id image unchanged; at SCALE_FIRST_BAD = ±32 the frames differ (test_scale_envelope_is_pinned)

@pytest.mark.parametrize("k", [-SCALE_K, -8, 8, SCALE_K])
def test_power_of_two_scale_is_invisible_in_the_oracle(P, pto, k):
    """Scaling every length by 2**k scales every step of SPEC §4-§5 by an exact power of two (only the leaf padding breaks the
    symmetry, which cannot change a hit), so the path-traced frame is bit-identical for every layout of the product's host
    builder. Catches what does not scale with the scene: an absolute distance constant in the oracle, or a quantiser exponent
    saturating at its clamp. A scale-invariant rounding error of the quantiser shifts with k in both frames; a box that no
    longer encloses its triangles is caught by test_oracle_closest_hit_matches_float64 instead."""
    N = P.native
    for sd in (P.make_scene(N.PT_SCENE_CORNELL, 0, 5, 48, 36), P.make_scene(N.PT_SCENE_CORNELL_GLASS, 0, 5, 48, 36),
               P.make_scene(N.PT_SCENE_CORNELL_TESS, 2000, 5, 48, 36)):
        p = P.make_params(48, 36, spp=2, max_depth=6)
        info, nodes, tris = build_bvh_detached(sd, 2)
        ref, ost = pto.render(pto.Scene(sd, (info.width, nodes, tris)), p)
        s2 = S.scaled(sd, k)
        p2 = P.make_params(48, 36, spp=2, max_depth=6, ray_eps=1e-4 * 2.0 ** k)
        for layout in LAYOUTS:
            info, nodes, tris = build_bvh_detached(s2, layout)
            img, st = pto.render(pto.Scene(s2, (info.width, nodes, tris)), p2)
            assert st.rays == ost.rays and np.array_equal(img, ref), (k, layout)


def test_scale_envelope_is_pinned(P, pto):
    """One step of 2 past the envelope the frame is no longer the unscaled one, at either end: §5's normalize(cross(e1, e2)) takes
    dot(cr, cr), a fourth-order product of lengths, which overflows at 2^32 for the Cornell walls (2^(4k+4) >= 2^128) and goes
    denormal at 2^-32 for the tessellated box's small triangles. The hit ids still hold there (geometry_space.HIT_K)."""
    N = P.native
    assert SCALE_FIRST_BAD == (-SCALE_K - 2, SCALE_K + 2)
    for k, kind, detail in ((SCALE_FIRST_BAD[1], N.PT_SCENE_CORNELL, 0), (SCALE_FIRST_BAD[0], N.PT_SCENE_CORNELL_TESS, 2000)):
        sd = P.make_scene(kind, detail, 5, 48, 36)
        frames = []
        for s, eps in ((sd, 1e-4), (S.scaled(sd, k), 1e-4 * 2.0 ** k)):
            info, nodes, tris = build_bvh_detached(s, 2)
            frames.append(pto.render(pto.Scene(s, (info.width, nodes, tris)), P.make_params(48, 36, spp=2, max_depth=6, ray_eps=eps))[0])
        assert not np.array_equal(frames[0], frames[1]), k


def test_shared_edge_leak_is_pinned(P, pto):
    """SPEC §4's Möller–Trumbore is not watertight: rays aimed at edges shared by two triangles of a closed mesh slip through.
    The count is pinned (brute force and the product's blob agree on every ray), so a watertight test shows up here."""
    sd, _, o, d = crack_rays(P, pto)
    info, nodes, tris = build_bvh_detached(sd, 0)
    bf, bvh = pto.Scene(sd), pto.Scene(sd, (info.width, nodes, tris))
    ids = np.array([bf.closest(o[i], d[i])[0] for i in range(len(o))], np.uint64)
    assert np.array_equal(ids, [bvh.closest(o[i], d[i])[0] for i in range(len(o))])
    c = rc.classify(sd.verts, sd.spheres, o, d, ids)
    assert len(c["wrong"]) == 0 and len(c["coincident"]) == 0
    assert (c["want"] != rc.MISS).all()  # in float64 every one of these rays hits the box
    assert len(c["crack"]) == int((ids == rc.MISS).sum()) == PINNED_CRACKS


@pytest.mark.xfail(strict=True, reason="SPEC §4's Möller–Trumbore test is not watertight: rays through shared edges of a closed "
                                       "mesh can miss both triangles (test_shared_edge_leak_is_pinned)")
def test_shared_edges_are_watertight(P, pto):
    sd, _, o, d = crack_rays(P, pto)
    bf = pto.Scene(sd)
    assert all(bf.closest(o[i], d[i])[0] != rc.MISS for i in range(len(o)))


@pytest.mark.xfail(strict=True, raises=AssertionError, reason="SPEC §4's discriminant b² − (|oc|² − r²) cancels: at 3000 radii its error, about (|oc|/r)² · 2^-24 "
                                       "= 0.5 r², is the size of the sphere, and 280 of 1728 rays of the fan disagree with float64 far "
                                       "outside EDGE_BAND. The well-conditioned form r² − |oc − b·d|² (which the caster uses) would turn this.")
def test_far_sphere_at_3000_radii_agrees_with_float64(P, pto):
    case = G.find("far_sphere_3000")
    o, d = case.rays
    ids, _, _ = oracle(pto, pto.Scene(case.sd), o, d)
    assert len(rc.classify(case.sd.verts, case.sd.spheres, o, d, ids)["wrong"]) == 0


def _scene_at_two_to_the_64(pto):
    """(unscaled ids, ids with every length times 2^64) of the glass box's camera rays, brute force."""
    sd = G.glass()
    o, d = rc.camera_rays(pto, sd.cam, G.W, G.H)
    want, _, _ = oracle(pto, pto.Scene(sd), o, d)
    got, _, _ = oracle(pto, pto.Scene(S.scaled(sd, 64)), o * np.float32(2.0 ** 64), d)
    return want, got


def test_scene_at_two_to_the_64_goes_empty(P, pto):
    """What the xfail below stands on: the unscaled box has 1190 hits of 1728 rays, the scaled one none, and no call fails."""
    want, got = _scene_at_two_to_the_64(pto)
    assert (want != rc.MISS).sum() == 1190 and (got == rc.MISS).all()


@pytest.mark.xfail(strict=True, raises=AssertionError, reason="Möller–Trumbore's third-order products dot(e2, cross(tv, e1)) ~ 2^(3k+4) overflow f32 long before "
                                       "the coordinates do: with every length times 2^64 no call fails and every ray misses. The domain "
                                       "is stated in SPEC §4 (2^±30 for frames, ids hold to 2^±40) rather than enforced.")
def test_scene_at_two_to_the_64_keeps_its_hits(P, pto):
    want, got = _scene_at_two_to_the_64(pto)
    assert np.array_equal(got, want)
