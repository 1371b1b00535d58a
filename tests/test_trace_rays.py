"""CPU checks of pt_trace_rays (include/ptrt.h, docs/SPEC.md §4.2): the export and its declared argument types, the calls refused
before any device is touched, and the §4.2 rule itself restated in numpy over the oracle's closest hit (pto.Scene.closest plus the
tmax filter), which must agree with the float64 ray caster away from edges and from the tmax boundary."""
import ctypes as C

import numpy as np

import adversarial_scenes as S
import ray_caster64 as rc
from float64_support import build_bvh_detached
from trace_support import MISS


def test_trace_rays_is_exported_with_the_documented_argtypes(P):
    N = P.native
    assert hasattr(N.lib, "pt_trace_rays")
    res, args = N.SYMBOLS["pt_trace_rays"]
    assert res is C.c_int32
    assert args == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(N.pt_stats)]
    assert N.lib.pt_trace_rays.argtypes == args
    assert (N.PT_TRACE_OCCLUSION, N.PT_TRACE_COUNT_VISITS, N.PT_TRACE_HOST_MEMORY) == (1, 2, 4)


def test_refused_without_a_device(P):
    N = P.native
    rays = np.zeros((4, 8), np.float32)
    hits = np.zeros((4, 4), np.float32)
    st = N.pt_stats()
    call = lambda ctx, scene, flags: N.lib.pt_trace_rays(ctx, scene, rays.ctypes.data_as(C.c_void_p), hits.ctypes.data_as(C.c_void_p),
                                                         4, flags, C.byref(st))
    assert call(None, None, N.PT_TRACE_HOST_MEMORY) == N.PT_ERR_INVALID_ARGUMENT
    assert b"NULL" in N.lib.pt_last_error(None)
    for bad in (8, 0x80000000):
        assert call(None, None, bad | N.PT_TRACE_HOST_MEMORY) == N.PT_ERR_INVALID_ARGUMENT
        assert b"unknown flag" in N.lib.pt_last_error(None)
    assert call(None, None, N.PT_TRACE_OCCLUSION | N.PT_TRACE_COUNT_VISITS) == N.PT_ERR_INVALID_ARGUMENT
    assert b"COUNT_VISITS" in N.lib.pt_last_error(None)
    # a detached (context-less) scene cannot be queried either
    sd = P.make_scene(N.PT_SCENE_CORNELL, 0, 1, 16, 16)
    s = C.c_void_p()
    assert N.lib.pt_scene_create(None, C.byref(s)) == N.PT_OK
    try:
        assert call(None, s, N.PT_TRACE_HOST_MEMORY) == N.PT_ERR_INVALID_ARGUMENT
    finally:
        N.lib.pt_scene_destroy(s)
    assert (hits == 0).all()
    del sd


def spec_trace(osc, o, d, tmax):
    """SPEC §4.2 closest-hit query restated: the oracle's unbounded closest hit, kept when t <= tmax (tmax <= 0 or NaN: a miss)."""
    ids, ts = np.empty(len(o), np.uint64), np.empty(len(o), np.float32)
    for i in range(len(o)):
        ids[i], ts[i] = osc.closest(o[i], d[i])
    with np.errstate(invalid="ignore"):
        keep = (ids != MISS) & (ts <= tmax) & (tmax > 0)
    return np.where(keep, ids, MISS).astype(np.uint64), np.where(keep, ts, np.inf).astype(np.float32)


def test_spec_rule_agrees_with_float64(P, pto):
    """The §4.2 rule on the oracle's hits equals the same rule applied to the float64 caster's hits, for random finite tmax, on rays
    that are clear of edges, of coincident surfaces and of the tmax boundary (relative 1e-4)."""
    N = P.native
    rng = np.random.default_rng(3)
    for sd in (P.make_scene(N.PT_SCENE_CORNELL_GLASS, 0, 3, 40, 30), P.make_scene(N.PT_SCENE_CORNELL_TESS, 2000, 3, 40, 30),
               S.duplicates(40, 30)[0]):
        info, nodes, tris = build_bvh_detached(sd, 68)
        osc = pto.Scene(sd, (info.width, nodes, tris))
        o, d = rc.camera_rays(pto, sd.cam, 40, 30)
        want, t64, edge, in_plane = rc.cast(sd.verts, sd.spheres, o, d)
        hit64 = want != MISS
        tmax = (rng.random(len(o)) * 2.0 * np.where(hit64, t64, 1.0)).astype(np.float32)
        tmax[::17] = np.inf
        tmax[5::31] = -1.0
        ids, ts = spec_trace(osc, o, d, tmax)
        want_q = np.where(hit64 & (t64 <= tmax) & (tmax > 0), want, MISS)
        with np.errstate(invalid="ignore"):
            clear = ~in_plane & ~(edge < 1e-5) & ~(hit64 & (np.abs(t64 - tmax) <= 1e-4 * t64))
        assert clear.sum() > 0.8 * len(o)
        assert np.array_equal(ids[clear], want_q[clear]), np.nonzero(ids[clear] != want_q[clear])[0][:8]
        both = clear & (ids != MISS)
        assert np.allclose(ts[both], t64[both], rtol=1e-5)
        assert (ts[ids == MISS] == np.inf).all() and ((ids == MISS) | (ts <= tmax)).all()
        assert (ids[tmax <= 0] == MISS).all() and 0 < (ids != MISS).sum() < len(o)
