"""-m gpu: the two visit orders of the traversal (docs/SPEC.md §4.1) against each other and against the oracle.

The counting kernels visit a node's hit children in the spec's order; the others enter the nearest child first and push the rest
unsorted (kernels.hip VisitOrder). The hit must not depend on it (§4), the visit counters belong to the counting kernels alone. So:
the plain query's hit records equal the counting query's bit for bit, whose sums equal the oracle's; plain frames equal the oracle's
frames bit for bit; occlusion answers what the closest hit answers; and a counting frame still reports the oracle's counters."""
import dataclasses

import numpy as np
import pytest

import adversarial_scenes as S
import float64_support as F
import ray_caster64 as rc
from frame_checks import assert_parity, check_nee, run_both
from trace_support import MISS, check_closest, commit, ids_of, oracle, records, same

pytestmark = pytest.mark.gpu

LAYOUTS = [4, 68, 72]   # four children, four quantised children, eight quantised children: the layouts with more than one comparator
MAX_RAYS = 8192
FW, FH = 96, 64          # the frames' size


def _bounce_records(sd, rec, hits, seed=7, eps=1e-4):
    """Cosine-distributed unit directions about the surface normal at every hit of `rec` (misses dropped), origins offset by eps
    along the normal: the incoherent rays a path's second vertex traces."""
    ids = ids_of(hits).astype(np.int64)
    ok = ids != MISS
    o, d, t, ids = rec[ok, 0:3], rec[ok, 4:7], hits[ok, 0:1], ids[ok]
    p = o + t * d
    v = np.asarray(sd.verts, np.float32).reshape(-1, 3, 3)
    n = np.zeros_like(p)
    tri = ids < len(v)
    n[tri] = np.cross(v[ids[tri], 1] - v[ids[tri], 0], v[ids[tri], 2] - v[ids[tri], 0])
    if (~tri).any():
        n[~tri] = p[~tri] - np.asarray(sd.spheres, np.float32).reshape(-1, 4)[ids[~tri] - len(v), :3]
    keep = np.linalg.norm(n, axis=1) > 0
    p, d, n = p[keep], d[keep], n[keep]
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n *= np.where((n * d).sum(1) < 0, 1.0, -1.0)[:, None].astype(np.float32)
    rng = np.random.default_rng(seed)
    u1, u2 = rng.random(len(p)), rng.random(len(p))
    a = np.where(np.abs(n[:, :1]) > 0.9, [[0, 1, 0]], [[1, 0, 0]]).astype(np.float32)
    tx = np.cross(n, a)
    tx /= np.linalg.norm(tx, axis=1, keepdims=True)
    ty = np.cross(n, tx)
    r, phi = np.sqrt(u1)[:, None], (2 * np.pi * u2)[:, None]
    dd = r * np.cos(phi) * tx + r * np.sin(phi) * ty + np.sqrt(1 - u1)[:, None] * n
    dd /= np.linalg.norm(dd, axis=1, keepdims=True)
    return records((p + eps * n).astype(np.float32), dd.astype(np.float32))


def _batch(pto, r, sd, w, h, stride):
    """Every `stride`-th camera ray of the scene plus the bounce rays from their hits (through the scene as `r` holds it)."""
    o, d = rc.camera_rays(pto, sd.cam, w, h)
    cam = records(o[::stride], d[::stride])
    rec = np.concatenate([cam, _bounce_records(sd, cam, r.TraceRays(cam)[0])])
    assert 0 < len(rec) <= MAX_RAYS, len(rec)
    return rec


def _ties(w, h):
    """S.duplicates with the vertices of every other copy rotated (as tests/test_gpu_bvh4q_parity.py builds it): ties on t, exact and
    up to the last bit, across leaves."""
    sd, _ = S.duplicates(w, h)
    v = sd.verts.reshape(-1, 3, 3).copy()
    v[1::2] = v[1::2][:, [1, 2, 0]]
    sd.verts = v.reshape(sd.verts.shape)
    return sd


def _cases(P):
    """(name, scene, frame size, camera-ray stride, builders)."""
    N = P.native
    both = (0, N.PT_BVH_BUILD_LBVH)
    out = [("tess20k", P.make_scene(N.PT_SCENE_CORNELL_TESS, 20000, 0x5EED0001, FW, FH), (FW, FH), 2, both),
           ("soup20k", P.make_scene(N.PT_SCENE_TRIANGLE_SOUP, 20000, 0x5EED0001, FW, FH), (FW, FH), 2, both)]
    for name, sd in F.scenes(P).items():
        out.append((name, sd, F._size(name), 3, (0,)))
    out.append(("ties", _ties(F.W, F.H), (F.W, F.H), 3, (0,)))
    return out


def test_both_orders_find_the_same_hits(P, pto, renderer):
    """pt_trace_rays without counting (nearest first) and with PT_TRACE_COUNT_VISITS (the spec's order) on camera and bounce rays:
    hit records (t, prim id, u, v) equal bit for bit, the counting run's hits and sums the oracle's. And occlusion on the same
    batch: occluded exactly where the closest-hit query with the same tmax hits."""
    rng = np.random.default_rng(19)
    for name, sd, (w, h), stride, builders in _cases(P):
        for width in LAYOUTS:
            for build in builders:
                ctx = (name, width, build)
                osc = commit(P, pto, renderer, sd, width | build)
                assert renderer.BvhInfo().width == width, ctx
                if name == "layers":  # the traversal stack's overflow columns are in use, under each layout's own visit order
                    assert renderer.BvhInfo().stack_need > 12, ctx
                rec = _batch(pto, renderer, sd, w, h, stride)
                plain, _ = renderer.TraceRays(rec)
                counted, st = renderer.TraceRays(rec, count_visits=True)
                assert same(plain, counted), (ctx, np.nonzero((plain.view(np.uint32) != counted.view(np.uint32)).any(axis=1))[0][:8])
                ids, ts, ost = oracle(pto, osc, rec[:, 0:3], rec[:, 4:7])
                check_closest(counted, ids, ts, ctx)
                assert (st.node_visits, st.tri_tests, st.sphere_tests) == (ost.node_visits, ost.tri_tests, ost.sphere_tests), ctx
                # occlusion against the closest hit under the same finite tmax (shadow rays carry one)
                hit = ids != MISS
                tm = (rng.random(len(rec)) * 2.0 * np.where(hit, ts, 1.0)).astype(np.float32)
                closest, _ = renderer.TraceRays(rec, tmax=tm)
                assert np.array_equal(ids_of(closest) != MISS, hit & (ts <= tm)), ctx
                occ, _ = renderer.TraceRays(rec, tmax=tm, occlusion=True)
                assert np.array_equal(ids_of(occ) != MISS, ids_of(closest) != MISS), ctx


@pytest.fixture(scope="module")
def soup(P):
    """5,000 random triangles: a node's boxes overlap, so three or more children are hit in many visits."""
    return P.make_scene(P.native.PT_SCENE_TRIANGLE_SOUP, 5000, 0x5EED0001, FW, FH)


def _soup_params(P, flags=0):
    p = P.make_params(FW, FH, spp=4, max_depth=8, streams=8)
    p.flags |= P.native.PT_FLAG_EXTEND_SIMPLE | flags
    return p


@pytest.mark.parametrize("width", LAYOUTS)
def test_plain_frames_are_the_oracles(P, pto, renderer, soup, width):
    """The one-ray-per-lane kernel, not counting: the frame equals the oracle's bit for bit, and so do the ray and path counts."""
    img, st, ref, ost = run_both(P, pto, renderer, soup, _soup_params(P), width)
    assert renderer.BvhInfo().width == width
    assert_parity(img, st, ref, ost)


def test_next_event_frames_are_the_checkers(P, pto, renderer, soup):
    """PT_FLAG_NEXT_EVENT on BVH4Q: shadow rays start with a tmax, so a node is culled against min(tfar, tmax) from the root on. The
    same frame of the soup with every 40th triangle a light (the generator's soup has none, and without lights no shadow ray is
    traced; few of its paths reach a surface at all), and the tessellated Cornell box under its ceiling light, where most vertices
    trace one: frames and ray counts are the checker's, and shadow rays were traced."""
    light = np.zeros(1, soup.mats.dtype)
    light["albedo"], light["emission"] = 0.5, (6.0, 5.0, 4.0)
    tri_mat = soup.tri_mat.copy()
    tri_mat[::40] = len(soup.mats)
    lit = dataclasses.replace(soup, mats=np.concatenate([soup.mats, light]), tri_mat=tri_mat)
    tess = P.make_scene(P.native.PT_SCENE_CORNELL_TESS, 3000, 0x5EED0001, FW, FH)  # the checker tests every triangle per ray
    params = _soup_params(P, P.native.PT_FLAG_NEXT_EVENT)
    for name, sd, least in (("soup5k with lights", lit, 100), ("tess3k", tess, FW * FH)):
        renderer.SetScene(sd, 68)
        renderer.Params = params
        st, cst = check_nee(P, pto, renderer, sd, params, name)
        assert cst.n_lights > 0 and cst.shadow_rays >= least, (name, cst.n_lights, cst.shadow_rays)
        assert st.rays == cst.ext_rays + cst.shadow_rays > cst.ext_rays, name


@pytest.mark.parametrize("width", LAYOUTS)
def test_counting_frames_keep_the_spec_order(P, pto, renderer, soup, width):
    """A PT_FLAG_COUNT_VISITS frame reports the oracle's node, triangle and sphere counts: the nearest-first order has not reached a
    counting kernel."""
    img, st, ref, ost = run_both(P, pto, renderer, soup, _soup_params(P), width, count=True)
    assert_parity(img, st, ref, ost)
    assert (st.node_visits, st.tri_tests, st.sphere_tests) == (ost.node_visits, ost.tri_tests, ost.sphere_tests)
