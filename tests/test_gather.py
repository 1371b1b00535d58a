"""CPU checks of pt_gather (include/ptrt.h, docs/SPEC.md §12): the export and its declared argument types, every refusal that needs no
device, in the documented order and each with its message, and the reference the GPU tests compare with (tests/gather_ref.py) held
against the float64 ray caster on every ray that float64 can settle."""
import ctypes as C

import numpy as np
import pytest

import gather_ref as G


def test_gather_is_exported_with_the_documented_argtypes(P):
    N = P.native
    assert hasattr(N.lib, "pt_gather")
    res, args = N.SYMBOLS["pt_gather"]
    assert res is C.c_int32
    assert args == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(N.pt_gather_params), C.POINTER(N.pt_stats)]
    assert N.lib.pt_gather.argtypes == args
    assert C.sizeof(N.pt_gather_params) == 32 and N.PT_GATHER_HOST_MEMORY == 1
    assert [f[0] for f in N.pt_gather_params._fields_] == ["samples", "seed", "sample_offset", "point_offset", "max_distance", "ray_eps", "flags", "pad"]
    assert N.lib.pt_abi_version() == 2


def test_refused_without_a_device(P):
    """The parameter checks come first, in the order of their fields, then the NULL check: a bad parameter block is reported even when
    everything else is missing too."""
    N = P.native
    pts = np.zeros((4, 8), np.float32)
    pts[:, 5] = 1.0
    out = np.zeros((4, 8), np.float32)
    st = N.pt_stats()
    host = N.PT_GATHER_HOST_MEMORY

    def call(ctx, scene, gp, points=pts, rows=out):
        return N.lib.pt_gather(ctx, scene, None if points is None else points.ctypes.data_as(C.c_void_p),
                               None if rows is None else rows.ctypes.data_as(C.c_void_p), 4, None if gp is None else C.byref(gp), C.byref(st))

    err = lambda: N.lib.pt_last_error(None)
    assert call(None, None, None) == N.PT_ERR_INVALID_ARGUMENT and b"params is NULL" in err()
    for bad in (2, 0x80000000, 2 | host):
        assert call(None, None, N.pt_gather_params(flags=bad)) == N.PT_ERR_INVALID_ARGUMENT and b"unknown flag" in err()
    assert call(None, None, N.pt_gather_params(samples=4097, flags=host)) == N.PT_ERR_INVALID_ARGUMENT and b"4096" in err()
    for bad in (-1.0, float("nan"), float("inf")):
        assert call(None, None, N.pt_gather_params(max_distance=bad, flags=host)) == N.PT_ERR_INVALID_ARGUMENT and b"max_distance" in err()
        assert call(None, None, N.pt_gather_params(ray_eps=bad, flags=host)) == N.PT_ERR_INVALID_ARGUMENT and b"ray_eps" in err()
    # in field order: flags before samples before max_distance before ray_eps
    assert call(None, None, N.pt_gather_params(flags=2, samples=5000, max_distance=-1.0, ray_eps=-1.0)) == N.PT_ERR_INVALID_ARGUMENT and b"unknown flag" in err()
    assert call(None, None, N.pt_gather_params(samples=5000, max_distance=-1.0, ray_eps=-1.0)) == N.PT_ERR_INVALID_ARGUMENT and b"4096" in err()
    assert call(None, None, N.pt_gather_params(max_distance=-1.0, ray_eps=-1.0)) == N.PT_ERR_INVALID_ARGUMENT and b"max_distance" in err()
    # a good block: now the pointers
    good = N.pt_gather_params(samples=4096, max_distance=0.0, ray_eps=0.0, flags=host)
    assert call(None, None, good) == N.PT_ERR_INVALID_ARGUMENT and b"pt_gather: NULL argument" in err()
    # a detached (context-less) scene cannot be gathered on either, with or without the arrays
    s = C.c_void_p()
    assert N.lib.pt_scene_create(None, C.byref(s)) == N.PT_OK
    try:
        assert call(None, s, good) == N.PT_ERR_INVALID_ARGUMENT and b"NULL argument" in err()
        assert call(None, s, good, points=None) == N.PT_ERR_INVALID_ARGUMENT and call(None, s, good, rows=None) == N.PT_ERR_INVALID_ARGUMENT
    finally:
        N.lib.pt_scene_destroy(s)
    assert (out == 0).all()


@pytest.mark.parametrize("name", ["glass", "tess"])
def test_reference_agrees_with_float64(P, pto, name):
    """gather_ref's visibility of every (point, sample) ray — the oracle's closest hit under the t <= tmax rule — equals the float64
    caster's on the rays that are clear: not within 1e-5 of an edge of the hit, not in a triangle's plane, the hit not within 1e-4
    relative of max_distance. More than 0.8 of the rays are clear, unbounded and with max_distance about half the box."""
    sd, pts, nrm, rays = G.case(P, pto, name)
    assert len(pts) >= 257 and rays.valid.all() and rays.d.shape == (len(pts), G.K, 3)
    assert np.abs(np.linalg.norm(rays.d.astype(np.float64), axis=2) - 1).max() < 1e-6
    assert ((rays.d * np.stack([G.unit_normal(n) for n in nrm])[:, None, :]).sum(2) > -1e-6).all()  # the normal's hemisphere
    cast = G.cast_rays(sd, rays)
    for md in (0.0, G.half_box(sd)):
        occluded, clear = G.clear_rays(rays, cast, md)
        V = G.visible(rays, md)
        assert clear.sum() > 0.8 * clear.size
        assert np.array_equal(V[clear], ~occluded[clear]), np.argwhere(clear & (V == occluded))[:8]
        assert 0 < V.sum() < V.size
    ref = G.gather(rays, G.half_box(sd), sky=(1.0, 2.0, 3.0))
    assert np.array_equal(ref["count"], G.visible(rays, G.half_box(sd)).sum(1)) and np.allclose(ref["E"], ref["visibility"][:, None] * [1.0, 2.0, 3.0])
    assert (np.linalg.norm(ref["bent"], axis=1) <= ref["visibility"] + 1e-12).all()


def test_reference_marks_invalid_points(P, pto):
    sd, pts, nrm, _ = G.case(P, pto, "glass")
    assert not G.valid_point([np.nan, 0, 0], [0, 1, 0]) and not G.valid_point([0, 0, 0], [np.inf, 0, 0]) and not G.valid_point([0, 0, 0], [0, 0, 0])
    assert not G.valid_point([0, 0, 0], [1e-30, 0, 0]) and not G.valid_point([0, 0, 0], [3e38, 3e38, 0]) and G.valid_point(pts[0], 4 * nrm[0])
    assert np.array_equal(G.unit_normal(4 * nrm[0]), G.unit_normal(nrm[0]))
