"""-m gpu: the node loop of the non-counting one-ray-per-lane kernels against the counting kernels and the oracle.

The non-counting kernels (k_extend<L, false, ..>, k_trace<L, 0>, k_trace<L, 2>) run the node and leaf phases behind wave-uniform
loop branches, with the step guard in the loop condition, and the four-child layouts pop without a branch when a visit's nearest
slot missed (kernels.hip trace_ray, node_visit_rows). The counting kernels keep the per-lane loops. Per lane both make the same
visits, so: the plain query's hit records equal the counting query's bit for bit, occlusion answers what the closest hit answers,
and plain frames equal the oracle's. The batches are built so that the lanes of one wave take every branch that differs: deep and
shallow stacks side by side, rays that hit no child of the root beside rays that do, a wave with a single live lane, ties."""
import dataclasses

import numpy as np
import pytest

import adversarial_scenes as S
import float64_support as F
import ray_caster64 as rc
from frame_checks import assert_parity, check_nee, run_both
from trace_support import LAYOUTS, MISS, ids_of, records, same

pytestmark = pytest.mark.gpu

FW, FH = 64, 64   # the frames' size
WAVE = 64


def _bounds(sd):
    pts = np.concatenate([np.asarray(sd.verts, np.float32).reshape(-1, 3), np.asarray(sd.spheres, np.float32).reshape(-1, 4)[:, :3]])
    return pts.min(0), pts.max(0)


def _away(sd, n):
    """Rays that start beyond the scene's bounds and run away from it: no child of the root is hit, so the first `cur` of such a
    lane comes from its empty stack. Every third one runs along an axis (zero direction components)."""
    lo, hi = _bounds(sd)
    o = np.tile(hi + (hi - lo) + 1.0, (n, 1)).astype(np.float32)
    d = np.tile(np.array([0.6, 0.64, 0.48], np.float32), (n, 1))
    d[::3] = (1.0, 0.0, 0.0)
    return records(o, d)


def _mixed(pto, sd, w, h):
    """The scene's camera rays and as many away rays, arranged so that the batch has waves of camera rays only, waves of away rays
    only, waves that alternate lane by lane, waves with one camera ray among away rays and waves whose other 63 lanes carry tmax = 0
    (pt_trace_rays traces nothing for them: one live lane); one ray more than a whole number of waves."""
    o, d = rc.camera_rays(pto, sd.cam, w, h)
    cam = records(o, d)
    n = len(cam) // (4 * WAVE) * (4 * WAVE)
    cam, away = cam[:n].copy(), _away(sd, n)
    q = n // 4
    lane = np.arange(q)
    alt = np.where((lane % 2 == 0)[:, None], cam[q:2 * q], away[q:2 * q])
    one = np.where((lane % WAVE == 17)[:, None], cam[2 * q:3 * q], away[2 * q:3 * q])
    dead = cam[3 * q:].copy()
    dead[np.arange(len(dead)) % WAVE != 40, 3] = 0.0
    return np.concatenate([cam[:q], away[:q], alt, one, dead, cam[:1]])


def _check_batch(renderer, rec, ctx, rng):
    plain, _ = renderer.TraceRays(rec)
    counted, _ = renderer.TraceRays(rec, count_visits=True)
    assert same(plain, counted), (ctx, np.nonzero((plain.view(np.uint32) != counted.view(np.uint32)).any(axis=1))[0][:8])
    hit = ids_of(counted) != MISS
    assert hit.any() and not hit.all(), ctx
    # occlusion against the closest hit under the same finite tmax
    tm = (rng.random(len(rec)) * 2.0 * np.where(hit, counted[:, 0], 1.0)).astype(np.float32)
    tm = np.where(rec[:, 3] > 0, tm, 0.0).astype(np.float32)
    closest, _ = renderer.TraceRays(rec, tmax=tm)
    closest_counted, _ = renderer.TraceRays(rec, tmax=tm, count_visits=True)
    assert same(closest, closest_counted), ctx
    occ, _ = renderer.TraceRays(rec, tmax=tm, occlusion=True)
    assert np.array_equal(ids_of(occ) != MISS, ids_of(closest) != MISS), ctx
    return hit


def _ties(w, h):
    """S.duplicates with the vertices of every other copy rotated: ties on t, exact and up to the last bit, across leaves."""
    sd, _ = S.duplicates(w, h)
    v = sd.verts.reshape(-1, 3, 3).copy()
    v[1::2] = v[1::2][:, [1, 2, 0]]
    sd.verts = v.reshape(sd.verts.shape)
    return sd


@pytest.mark.parametrize("width", LAYOUTS)
def test_plain_queries_are_the_counting_queries(P, pto, renderer, width):
    """Mixed batches on the deep-tree scene (lanes past kStackLds beside lanes with an empty stack), the tessellated Cornell box
    and the tie scene: closest-hit records of the plain and the counting query bit for bit, and occlusion."""
    rng = np.random.default_rng(width)
    for name, sd in (("layers", S.stacked_layers(F.W, F.H)), ("tess", P.make_scene(P.native.PT_SCENE_CORNELL_TESS, 2000, 5, F.W, F.H)),
                     ("ties", _ties(F.W, F.H))):
        renderer.SetScene(sd, width)
        assert renderer.BvhInfo().width == width, (name, width)
        if name == "layers" and width in (4, 68, 72):  # the overflow columns of the traversal stack are in use
            assert renderer.BvhInfo().stack_need > 12, (name, width)
        rec = _mixed(pto, sd, F.W, F.H)
        assert len(rec) % WAVE == 1
        hit = _check_batch(renderer, rec, (name, width), rng)
        q = (len(rec) - 1) // 5
        assert not hit[q:2 * q].any(), (name, width)            # the away rays hit nothing
        assert not hit[4 * q:5 * q][np.arange(q) % WAVE != 40].any()  # nor do rays with tmax = 0


@pytest.fixture(scope="module")
def soup(P):
    """5,000 random triangles: a node's boxes overlap, so three or more children are hit in many visits."""
    return P.make_scene(P.native.PT_SCENE_TRIANGLE_SOUP, 5000, 0x5EED0001, FW, FH)


def _soup_params(P, flags=0):
    p = P.make_params(FW, FH, spp=2, max_depth=8, streams=8)
    p.flags |= P.native.PT_FLAG_EXTEND_SIMPLE | flags
    return p


@pytest.mark.parametrize("width", LAYOUTS)
def test_plain_frames_are_the_oracles(P, pto, renderer, soup, width):
    """The one-ray-per-lane kernel, not counting, on the soup at 64 x 64 and 2 spp (paths end at every depth: queue holes, waves
    with few live lanes): frame, ray count and path count are the oracle's."""
    img, st, ref, ost = run_both(P, pto, renderer, soup, _soup_params(P), width)
    assert renderer.BvhInfo().width == width
    assert_parity(img, st, ref, ost)


def test_next_event_frame_is_the_checkers(P, pto, renderer, soup):
    """PT_FLAG_NEXT_EVENT on BVH4Q: shadow rays enter the node loop with a tmax. The soup with every 40th triangle a light."""
    light = np.zeros(1, soup.mats.dtype)
    light["albedo"], light["emission"] = 0.5, (6.0, 5.0, 4.0)
    tri_mat = soup.tri_mat.copy()
    tri_mat[::40] = len(soup.mats)
    lit = dataclasses.replace(soup, mats=np.concatenate([soup.mats, light]), tri_mat=tri_mat)
    params = _soup_params(P, P.native.PT_FLAG_NEXT_EVENT)
    renderer.SetScene(lit, 68)
    renderer.Params = params
    st, cst = check_nee(P, pto, renderer, lit, params, "soup5k with lights")
    assert cst.n_lights > 0 and cst.shadow_rays > 0, (cst.n_lights, cst.shadow_rays)
    assert st.rays == cst.ext_rays + cst.shadow_rays > cst.ext_rays
