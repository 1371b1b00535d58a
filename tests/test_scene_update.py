"""CPU checks of pt_scene_update_triangles / pt_scene_update_spheres (include/ptrt.h, docs/SPEC.md §4.3): the exports, the ctypes
signatures against the header, the ABI version, and every refusal that needs no device — on detached (context-less) scenes, which
pass the argument checks and are then refused as PT_ERR_UNSUPPORTED."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exported_and_abi_unchanged(P):
    N = P.native
    assert N.lib.pt_abi_version() == 2 == N.PTRT_ABI_VERSION
    for name in ("pt_scene_update_triangles", "pt_scene_update_spheres"):
        assert hasattr(N.lib, name), name
    assert N.PT_UPDATE_HOST_MEMORY == 1


def test_signatures_match_the_header(P):
    N = P.native
    res, args = N.SYMBOLS["pt_scene_update_triangles"]
    assert res is C.c_int32 and args == [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(N.pt_stats)]
    assert N.lib.pt_scene_update_triangles.argtypes == args
    res, args = N.SYMBOLS["pt_scene_update_spheres"]
    assert res is C.c_int32 and args == [C.c_void_p, C.c_void_p, C.c_uint64]
    assert N.lib.pt_scene_update_spheres.argtypes == args
    header = open(os.path.join(ROOT, "include", "ptrt.h")).read()
    assert re.search(r"pt_status pt_scene_update_triangles\(pt_scene \*s, const void \*verts9, uint64_t count, uint32_t flags, pt_stats \*stats\);", header)
    assert re.search(r"pt_status pt_scene_update_spheres\(pt_scene \*s, const float \*cxyzr, uint64_t count\);", header)
    assert re.search(r"PT_UPDATE_HOST_MEMORY = 1u", header)


def _detached(P, sd, commit=True):
    N = P.native
    s = C.c_void_p()
    assert N.lib.pt_scene_create(None, C.byref(s)) == N.PT_OK
    keep = [np.ascontiguousarray(sd.verts, np.float32), np.ascontiguousarray(sd.tri_mat, np.uint32),
            np.ascontiguousarray(sd.spheres, np.float32), np.ascontiguousarray(sd.sph_mat, np.uint32), np.ascontiguousarray(sd.mats)]
    p = [a.ctypes.data_as(C.c_void_p) for a in keep]
    assert N.lib.pt_scene_set_triangles(s, p[0], p[1], len(keep[1])) == N.PT_OK
    assert N.lib.pt_scene_set_spheres(s, p[2], p[3], len(keep[3])) == N.PT_OK
    assert N.lib.pt_scene_set_materials(s, p[4], len(keep[4])) == N.PT_OK
    assert N.lib.pt_scene_set_camera(s, C.byref(sd.cam)) == N.PT_OK
    if commit:
        assert N.lib.pt_scene_commit(s, 68) == N.PT_OK
    return s


def test_refusals(P):
    """NULL scene, unknown flags, an uncommitted scene, a wrong count, NULL vertices, non-finite host vertices, a bad sphere and a
    detached scene each return their documented status, and the detached scene's blob is untouched by all of them."""
    N = P.native
    sd = P.make_scene(N.PT_SCENE_CORNELL_GLASS, 0, 1, 16, 16)
    nt, ns = len(sd.tri_mat), len(sd.sph_mat)
    assert nt > 0 and ns > 0
    v = np.ascontiguousarray(sd.verts, np.float32).copy()
    sph = np.ascontiguousarray(sd.spheres, np.float32).copy()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    st = N.pt_stats()
    upd = lambda s, verts, n, flags=N.PT_UPDATE_HOST_MEMORY: N.lib.pt_scene_update_triangles(s, verts, n, flags, C.byref(st))
    ups = lambda s, a, n: N.lib.pt_scene_update_spheres(s, a, n)

    assert upd(None, ptr(v), nt) == N.PT_ERR_INVALID_ARGUMENT
    assert ups(None, ptr(sph), ns) == N.PT_ERR_INVALID_ARGUMENT

    fresh = _detached(P, sd, commit=False)
    try:
        assert upd(fresh, ptr(v), nt) == N.PT_ERR_NOT_COMMITTED
        assert ups(fresh, ptr(sph), ns) == N.PT_ERR_NOT_COMMITTED
    finally:
        N.lib.pt_scene_destroy(fresh)

    s = _detached(P, sd)
    try:
        info = N.pt_bvh_info()
        assert N.lib.pt_scene_bvh_info(s, C.byref(info)) == N.PT_OK
        before = [np.zeros(int(info.node_bytes), np.uint8), np.zeros(int(info.tri_bytes), np.uint8)]
        assert N.lib.pt_scene_bvh_read(s, ptr(before[0]), info.node_bytes, ptr(before[1]), info.tri_bytes) == N.PT_OK
        for bad in (2, 0x80000000):
            assert upd(s, ptr(v), nt, bad | N.PT_UPDATE_HOST_MEMORY) == N.PT_ERR_INVALID_ARGUMENT
            assert b"unknown flag" in N.lib.pt_last_error(None)
        for n in (nt - 1, nt + 1, 0):
            assert upd(s, ptr(v), n) == N.PT_ERR_INVALID_ARGUMENT
        assert upd(s, None, nt) == N.PT_ERR_INVALID_ARGUMENT
        assert b"NULL" in N.lib.pt_last_error(None)
        for value in (np.nan, np.inf, -np.inf):
            w = v.copy()
            w.reshape(-1)[7] = value
            assert upd(s, ptr(w), nt) == N.PT_ERR_INVALID_ARGUMENT
            assert b"non-finite" in N.lib.pt_last_error(None)
        assert upd(s, ptr(v), nt) == N.PT_ERR_UNSUPPORTED          # valid arguments: a detached scene has no device tree
        assert upd(s, ptr(v), nt, 0) == N.PT_ERR_UNSUPPORTED       # (device input is refused before its pointer is looked at)
        for n in (ns - 1, ns + 1):
            assert ups(s, ptr(sph), n) == N.PT_ERR_INVALID_ARGUMENT
        assert ups(s, None, ns) == N.PT_ERR_INVALID_ARGUMENT
        for k, value in ((3, 0.0), (3, -1.0), (3, np.inf), (0, np.nan)):
            w = sph.copy()
            w[1, k] = value
            assert ups(s, ptr(w), ns) == N.PT_ERR_INVALID_ARGUMENT
        assert ups(s, ptr(sph), ns) == N.PT_ERR_UNSUPPORTED
        after = [np.zeros_like(before[0]), np.zeros_like(before[1])]
        assert N.lib.pt_scene_bvh_read(s, ptr(after[0]), info.node_bytes, ptr(after[1]), info.tri_bytes) == N.PT_OK
        assert all(np.array_equal(a, b) for a, b in zip(before, after))
    finally:
        N.lib.pt_scene_destroy(s)


def test_python_wrapper_refuses_without_a_device(P):
    """Renderer.UpdateGeometry raises PtException for a renderer without a scene (no device needed to get there)."""
    import pytest
    r = P.Renderer(P.Window(8, 8))
    try:
        with pytest.raises(P.PtException):
            r.UpdateGeometry(verts=np.zeros((1, 9), np.float32))
        with pytest.raises(P.PtException):
            r.UpdateGeometry(spheres=np.ones((1, 4), np.float32))
    finally:
        r.Dispose()
