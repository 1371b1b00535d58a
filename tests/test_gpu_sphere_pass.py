"""-m gpu: the sphere list (kernels.hip spheres_test) against the oracle, bit for bit, on lists built to break a merged root pass.

spheres_test walks the list four spheres per 64-byte scalar load and runs sphere_test on each. A form that computes (b, disc) of a
chunk's four spheres first and then runs ONE copy of the square root, the root select and the accept rule in passes, each lane on the
lowest sphere whose line it still has to look at, was built and measured and is not kept; these tests were written for
it and hold whatever form the list takes. What such a form can get wrong is which sphere a lane takes in which pass, the pair it
recomputes for a second, third and fourth one, the end of the list inside a chunk, and the order-independence of the accept rule on
ties. The master list below is built so that single rays cross the lines of two, three and four spheres of one chunk and of two
chunks: concentric spheres, exact duplicates inside a chunk and across the chunk border (equal t: the lower id must win), a sphere
behind every origin, origins inside up to three spheres, and rays tangent to a sphere (disc == 0 exactly, and the first float
inside). Lists of 0, 1, 3, 4, 5, 8 and 9 spheres are prefixes of it, with and without triangles around them.

Part 1 asks pt_trace_rays (closest hit, counting, occlusion, tmax at a sphere's own t and one float below it); part 2 renders 64x48
frames at 4 spp through the one-ray-per-lane, the lane-packing and the pooled extend kernels and compares them with pto.render."""
import numpy as np
import pytest

import material_zoo as mz
from pipelines import named_flags
from trace_support import MISS, check_closest, commit, ids_of, oracle, records, same

pytestmark = pytest.mark.gpu

COUNTS = [0, 1, 3, 4, 5, 8, 9]
SPHERE_PASS_LAYOUTS = [2, 68, 73]
W, H = 64, 48
CASES = [(n, t) for n in COUNTS for t in (True, False) if n or t]  # lists with and without triangles around them (not the empty scene)
CASE_IDS = [f"{n}-{'tris' if t else 'no_tris'}" for n, t in CASES]

# id k of the list is sphere k (after the triangles). Chunk 0 = spheres 0-3, chunk 1 = 4-7, chunk 2 = 8.
MASTER = np.array([
    (0.0, 0.0, 0.0, 0.5),     # 0
    (0.0, 0.0, 0.0, 0.3),     # 1: concentric, inside 0
    (0.0, 0.0, 0.0, 0.5),     # 2: duplicate of 0, same chunk: every hit of it ties with 0, and 0 must keep it
    (0.0, 0.0, -1.5, 0.4),    # 3: further down the axis
    (0.0, 0.0, -1.5, 0.4),    # 4: duplicate of 3 across the chunk border
    (0.25, 0.0, 3.0, 0.6),    # 5: behind every origin of the axis rays and of the frames' camera
    (0.0, 0.0, -1.5, 0.2),    # 6: concentric, inside 3 and 4
    (0.1, -0.1, -3.0, 1.0),   # 7: a big one behind them all
    (0.0, 0.0, 0.0, 0.5),     # 8: duplicate of 0 and 2 in a third chunk
], np.float32)


def build_scene(n, with_tris):
    """The first `n` spheres of MASTER, materials of every kind on them (one emits), a Lambert floor and back wall or no triangle."""
    mats = [mz.mat(mz.LAMBERT, (0.8, 0.7, 0.6)), mz.mat(mz.LAMBERT, (0.2, 0.9, 0.3), emission=(3.0, 2.0, 1.0)),
            mz.mat(mz.METAL, (0.9, 0.8, 0.6), roughness=0.2), mz.mat(mz.LAMBERT, (0.9, 0.2, 0.2)),
            mz.mat(mz.DIELECTRIC, (1.0, 1.0, 1.0), ior=1.5), mz.mat(mz.LAMBERT, (0.3, 0.3, 0.9)),
            mz.mat(mz.LAMBERT, (0.7, 0.7, 0.7))]  # 6: the triangles
    tris, tm = [], []
    if with_tris:
        tris += mz.quad((-4, -1.3, -5), (0, 0, 9), (8, 0, 0)); tm += [6, 6]   # floor, normal +y
        tris += mz.quad((-4, -1.3, -4.6), (8, 0, 0), (0, 6, 0)); tm += [6, 6]  # back wall, normal +z
    cam = mz.camera((0.45, 0.35, 2.2), (0.0, -0.1, -1.0), fov_deg=55)
    return mz.scene(tris, tm, MASTER[:n], [k % 6 for k in range(n)], mats, cam, (0.5, 0.6, 0.8))


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def rays():
    """About 3400 rays: a grid of rays down the axis all spheres but one sit on (the lines of up to eight spheres each), tangents,
    origins inside the concentric groups, origins past everything looking away, and incoherent rays through the whole scene."""
    rng = np.random.default_rng(2024)
    g = np.linspace(-0.62, 0.62, 25, dtype=np.float32)
    gx, gy = np.meshgrid(g, g)
    n = gx.size
    axis_o = np.stack([gx.ravel(), gy.ravel(), np.full(n, 2.0, np.float32)], 1)
    axis_d = np.tile(np.float32([0, 0, -1]), (n, 1))
    # tangents of sphere 0 (radius 0.5) and of 3 (0.4): x exactly the radius gives disc == 0, a miss; the float below it a hit
    tx = np.float32([0.5, np.nextafter(np.float32(0.5), np.float32(0)), np.nextafter(np.float32(0.5), np.float32(1)),
                     0.4, np.nextafter(np.float32(0.4), np.float32(0)), -0.5, 0.3, np.nextafter(np.float32(0.3), np.float32(0))])
    tan_o = np.concatenate([np.stack([tx, np.zeros_like(tx), np.full_like(tx, 2.0)], 1),
                            np.stack([np.zeros_like(tx), tx, np.full_like(tx, 2.0)], 1)])
    tan_d = np.tile(np.float32([0, 0, -1]), (len(tan_o), 1))
    m = 500
    in_a = (rng.uniform(-0.28, 0.28, (m, 3))).astype(np.float32)                      # inside 0, 1, 2 (and 8), mostly inside 1
    in_b = (np.float32([0, 0, -1.5]) + rng.uniform(-0.22, 0.22, (m, 3))).astype(np.float32)  # inside 3, 4, around 6
    in_c = (np.float32([0.1, -0.1, -3.0]) + rng.uniform(-0.5, 0.5, (m, 3))).astype(np.float32)  # inside 7
    in_d = _unit(rng.normal(size=(3 * m, 3)))
    away_o = np.stack([rng.uniform(-0.5, 0.5, m), rng.uniform(-0.5, 0.5, m), np.full(m, 4.5)], 1).astype(np.float32)
    away_d = _unit(np.stack([rng.normal(size=m) * 0.3, rng.normal(size=m) * 0.3, np.ones(m)], 1))  # everything is behind
    box_o = np.stack([rng.uniform(-1, 1, 2 * m), rng.uniform(-1, 1, 2 * m), rng.uniform(-4.2, 4.2, 2 * m)], 1).astype(np.float32)
    aim = np.stack([rng.uniform(-0.4, 0.4, 2 * m), rng.uniform(-0.4, 0.4, 2 * m), rng.uniform(-3.5, 3.2, 2 * m)], 1)
    box_d = _unit(aim - box_o)                                                       # towards the axis: several lines each
    o = np.concatenate([axis_o, tan_o, in_a, in_b, in_c, away_o, box_o])
    d = np.concatenate([axis_d, tan_d, in_d, away_d, box_d])
    return np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)


@pytest.fixture(scope="module")
def ray_set():
    return rays()


def test_the_rays_cross_what_they_are_meant_to(ray_set):
    """The premise of this file, checked in float64 on the host: rays cross the lines of 2, 3 and 4 spheres of one chunk and lines in
    two chunks, some start inside spheres, some have every sphere behind them, and the tangent rays sit on disc == 0."""
    o, d = (a.astype(np.float64) for a in ray_set)
    c, r = MASTER[:, :3].astype(np.float64), MASTER[:, 3].astype(np.float64)
    oc = o[:, None, :] - c[None]
    b = (oc * d[:, None, :]).sum(-1)
    cc = (oc * oc).sum(-1) - r * r
    crossed = b * b - cc > 0
    per_chunk0, per_chunk1 = crossed[:, 0:4].sum(1), crossed[:, 4:8].sum(1)
    for k in (2, 3, 4):
        assert (per_chunk0 == k).sum() >= 20, k
    assert ((per_chunk0 >= 2) & (per_chunk1 >= 2)).sum() >= 200      # several lines in each of two chunks
    assert ((cc < 0).sum(1) >= 3).sum() >= 100                       # origins inside three spheres
    behind = crossed & (b > 0) & (cc > 0)                            # both roots negative
    assert (crossed.any(1) & (behind == crossed).all(1)).sum() >= 100  # every crossed sphere is behind the origin
    o32, d32 = ray_set
    oc32 = o32[625] - MASTER[0, :3]                                  # the first tangent ray, in binary32 as sphere_test does it
    b32 = np.float32(oc32 @ d32[625])
    assert b32 * b32 - (np.float32(oc32 @ oc32) - np.float32(0.25)) == 0


@pytest.mark.parametrize("n,with_tris", CASES, ids=CASE_IDS)
def test_trace_rays(P, pto, renderer, ray_set, n, with_tris):
    """pt_trace_rays on every layout: closest hits (t bits and id) and the three counters equal pto_closest's; tmax equal to the hit's
    own t keeps it and the float below loses it (closest hit and occlusion); the plain and the counting kernel agree."""
    sd = build_scene(n, with_tris)
    o, d = ray_set
    rec = records(o, d)
    want = None
    for layout in SPHERE_PASS_LAYOUTS if with_tris else SPHERE_PASS_LAYOUTS[:1]:
        osc = commit(P, pto, renderer, sd, layout)
        ctx = (n, with_tris, layout)
        ids, ts, ost = oracle(pto, osc, o, d)
        if want is None:
            want = ids
            n_tri = len(sd.tri_mat)
            hit_sphere = (ids >= n_tri) & (ids != MISS)
            if n:
                assert hit_sphere.sum() > 300, ctx
            if n >= 3:
                assert not (ids == n_tri + 2).any(), ctx             # the duplicate never takes a tie from sphere 0
            if n >= 5:
                assert (ids == n_tri + 3).any() and not (ids == n_tri + 4).any(), ctx
            if n == 9:
                assert not (ids == n_tri + 8).any(), ctx
        assert np.array_equal(ids, want), ctx                        # the layout does not change the closest hit
        hits, st = renderer.TraceRays(rec, count_visits=True)
        check_closest(hits, ids, ts, ctx)
        assert st.rays == len(o)
        assert (st.node_visits, st.tri_tests, st.sphere_tests) == (ost.node_visits, ost.tri_tests, ost.sphere_tests), ctx
        assert st.sphere_tests == n * len(o), ctx
        assert same(renderer.TraceRays(rec)[0], hits), ctx
        hit = ids != MISS
        tm = np.where(hit, ts, np.float32(1.0))
        below = np.nextafter(tm, np.float32(0))
        h2, _ = renderer.TraceRays(rec, tmax=tm)
        assert same(h2[hit], hits[hit]) and (ids_of(h2)[~hit] == MISS).all(), ctx
        h3, _ = renderer.TraceRays(rec, tmax=below)
        assert (ids_of(h3) == MISS).all(), ctx
        for tq, occluded in ((np.float32(np.inf), hit), (tm, hit), (below, np.zeros_like(hit))):
            h4, _ = renderer.TraceRays(rec, tmax=tq, occlusion=True)
            occ = ids_of(h4) != MISS
            assert np.array_equal(occ, occluded), ctx
            assert (ids_of(h4)[occ] < len(sd.tri_mat) + n).all() and (h4[occ, 0] > 0).all(), ctx
            assert (h4[occ, 0] <= np.broadcast_to(tq, occ.shape)[occ]).all() and (h4[:, 2:] == 0).all(), ctx


@pytest.mark.parametrize("n,with_tris", CASES, ids=CASE_IDS)
def test_frames(P, pto, renderer, n, with_tris):
    """64x48 frames at 4 spp (jitter on, every material kind on the spheres) through the three extend kernels: the oracle's picture,
    rays and paths."""
    N = P.native
    sd = build_scene(n, with_tris)
    sd.cam.jitter = 1
    for layout in (0, 68):
        renderer.SetScene(sd, layout)
        osc = pto.Scene(sd, (renderer.BvhInfo().width,) + renderer.BvhRead())
        ref = None
        for name, flag in named_flags("simple", "packed", "pool"):
            params = P.make_params(W, H, spp=4, max_depth=8, streams=2, flags=flag)
            if ref is None:
                ref, ost = pto.render(osc, params)
            renderer.Params = params
            st = renderer.Render(0.0)
            img = renderer.ReadFramebuffer()
            assert np.array_equal(img, ref), (n, with_tris, layout, name, int((img != ref).any(axis=2).sum()))
            assert (st.rays, st.paths) == (ost.rays, ost.paths), (n, with_tris, layout, name)
