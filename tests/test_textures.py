"""Albedo textures (docs/SPEC.md §13) without a device: the three setters and pt_scene_texture_info on detached scenes, the commit's
refusals, pipeline.h's decode with has_textures over every input, the scalar checker of tests/tex_ref/ against the oracle bit for bit, and
hand-computed answers of its lookup. tests/test_gpu_textures.py holds the device to the same checker."""
import ctypes as C
import dataclasses
import itertools
import os

import numpy as np
import pytest

import env_checker as ec
import tex_checker as tc
from pipelines import FLAGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 48, 36
PT_ERR_INVALID_ARGUMENT, PT_ERR_UNSUPPORTED = 1, 6


# ------------------------------------------------------------------------------------------------------------------------ the setters
class Detached:
    """A context-less scene (host side only) holding the Cornell box."""

    def __init__(self, P):
        self.P, self.N = P, P.native
        self.s = C.c_void_p()
        assert self.N.lib.pt_scene_create(None, C.byref(self.s)) == 0
        self.sd = P.make_scene(self.N.PT_SCENE_CORNELL, 0, 3, W, H)
        self.keep = [np.ascontiguousarray(self.sd.verts, np.float32), np.ascontiguousarray(self.sd.tri_mat, np.uint32),
                     np.ascontiguousarray(self.sd.spheres, np.float32), np.ascontiguousarray(self.sd.sph_mat, np.uint32),
                     np.ascontiguousarray(self.sd.mats)]
        v, tm, sp, sm, m = self.keep
        L, p = self.N.lib, lambda a: a.ctypes.data_as(C.c_void_p)
        assert L.pt_scene_set_triangles(self.s, p(v), p(tm), len(tm)) == 0 and L.pt_scene_set_spheres(self.s, p(sp), p(sm), len(sm)) == 0
        assert L.pt_scene_set_materials(self.s, p(m), len(m)) == 0 and L.pt_scene_set_camera(self.s, C.byref(self.sd.cam)) == 0

    def uvs(self, a):
        a = None if a is None else np.ascontiguousarray(a, np.float32)
        return self.N.lib.pt_scene_set_triangle_uvs(self.s, None if a is None else a.ctypes.data_as(C.c_void_p), 0 if a is None else len(a.reshape(-1, 6)))

    def texture(self, index, img, flags=0, w=None, h=None):
        a = None if img is None else np.ascontiguousarray(img, np.float32)
        return self.N.lib.pt_scene_set_texture(self.s, index, None if a is None else a.ctypes.data_as(C.c_void_p),
                                               (0 if a is None else a.shape[1]) if w is None else w, (0 if a is None else a.shape[0]) if h is None else h, flags)

    def binding(self, a):
        a = None if a is None else np.ascontiguousarray(a, np.uint32)
        return self.N.lib.pt_scene_set_material_textures(self.s, None if a is None else a.ctypes.data_as(C.c_void_p), 0 if a is None else len(a))

    def info(self, index):
        i = self.N.pt_texture_info()
        st = self.N.lib.pt_scene_texture_info(self.s, index, C.byref(i))
        return st, i

    def commit(self):
        return self.N.lib.pt_scene_commit(self.s, 0)

    def close(self):
        self.N.lib.pt_scene_destroy(self.s)


@pytest.fixture
def det(P):
    d = Detached(P)
    yield d
    d.close()


def test_constants_and_struct(P):
    N = P.native
    assert (N.PT_MAX_TEXTURES, N.PT_NO_TEXTURE, N.PT_TEXTURE_NEAREST) == (64, 0xFFFFFFFF, 1) and C.sizeof(N.pt_texture_info) == 24
    hdr = open(os.path.join(ROOT, "include", "ptrt.h")).read()
    assert "#define PT_MAX_TEXTURES 64u" in hdr and "#define PT_NO_TEXTURE 0xFFFFFFFFu" in hdr and "PT_TEXTURE_NEAREST = 1u" in hdr
    assert "#define PTRT_ABI_VERSION 2" in hdr
    for f in ("host/cpp/ptrt_host.hpp", "host/csharp/HipRenderer.cs"):
        txt = open(os.path.join(ROOT, f)).read()
        assert "pt_scene_set_triangle_uvs" in txt and "pt_scene_set_texture" in txt and "pt_scene_set_material_textures" in txt, f


def test_texture_setter_refusals_keep_the_previous_state(det):
    tex = tc.distinct(3, 5)
    assert det.info(7)[1].width == 0
    assert det.texture(7, tex, tc.NEAREST) == 0
    st, i = det.info(7)
    assert st == 0 and (i.width, i.height, i.flags, i.materials, i.device_bytes) == (3, 5, 1, 0, 0)
    bad = tex.copy()
    refusals = [det.texture(64, tex), det.texture(7, tex, 2), det.texture(7, tex, 3), det.texture(7, tex, w=0, h=5), det.texture(7, tex, w=3, h=0),
                det.texture(7, tex, w=4097, h=1), det.texture(7, tex, w=1, h=4097), det.texture(7, None, w=3, h=5), det.texture(7, None, flags=1)]
    for v in (-1.0, np.nan, np.inf, -0.0 - 1e-30):
        bad[2, 1, 1] = v
        refusals.append(det.texture(7, bad))
    assert refusals == [PT_ERR_INVALID_ARGUMENT] * len(refusals), refusals
    st, i = det.info(7)
    assert (i.width, i.height, i.flags) == (3, 5, 1)  # every refused call kept it
    assert det.info(64)[0] == PT_ERR_INVALID_ARGUMENT
    assert det.texture(7, np.zeros((1, 1, 3), np.float32)) == 0 and det.info(7)[1].width == 1 and det.info(7)[1].flags == 0  # zero is a texel
    assert det.texture(7, np.zeros((2, 4096, 3), np.float32)) == 0 and det.info(7)[1].width == 4096
    assert det.texture(7, None) == 0 and det.info(7)[1].width == 0  # removed


def test_uv_and_binding_setter_refusals(det):
    n = len(det.sd.tri_mat)
    uv = tc.planar_uvs(det.sd.verts)
    assert det.uvs(uv) == 0
    for v in (np.nan, np.inf, -np.inf, 1048577.0, -1048577.0):
        bad = uv.copy()
        bad[n - 1, 5] = v
        assert det.uvs(bad) == PT_ERR_INVALID_ARGUMENT, v
    edge = uv.copy()
    edge[0, 0], edge[0, 1] = 1048576.0, -1048576.0  # the bound itself is accepted
    assert det.uvs(edge) == 0
    assert det.N.lib.pt_scene_set_triangle_uvs(det.s, None, 3) == PT_ERR_INVALID_ARGUMENT
    assert det.binding([0, 64, 0, 0, 0, 0]) == PT_ERR_INVALID_ARGUMENT and det.binding([0xFFFFFFFE] * 6) == PT_ERR_INVALID_ARGUMENT
    assert det.N.lib.pt_scene_set_material_textures(det.s, None, 2) == PT_ERR_INVALID_ARGUMENT
    assert det.binding([tc.NO_TEXTURE] * 6) == 0 and det.binding([63, tc.NO_TEXTURE, 0, 0, 0, 0]) == 0  # (whether 63 is set is the commit's to say)
    for f in (det.N.lib.pt_scene_set_triangle_uvs, det.N.lib.pt_scene_set_material_textures):
        assert f(None, None, 0) == PT_ERR_INVALID_ARGUMENT
    assert det.N.lib.pt_scene_set_texture(None, 0, None, 0, 0, 0) == PT_ERR_INVALID_ARGUMENT


def test_commit_refusals_and_what_textured_means(det):
    """A count mismatch and a binding to a texture that is not set are the commit's refusals: the setters may come in any order. A refused
    setter call in between keeps the state that commits."""
    n, nm = len(det.sd.tri_mat), len(det.sd.mats)
    uv = tc.planar_uvs(det.sd.verts)
    assert det.commit() == 0  # nothing set
    assert det.uvs(uv[:-1]) == 0 and det.commit() == PT_ERR_INVALID_ARGUMENT  # one triangle short
    assert b"triangle" in det.N.lib.pt_last_error(None)
    assert det.uvs(np.concatenate([uv, uv[:1]])) == 0 and det.commit() == PT_ERR_INVALID_ARGUMENT
    assert det.uvs(uv) == 0 and det.commit() == 0
    assert det.binding([0] * (nm - 1)) == 0 and det.commit() == PT_ERR_INVALID_ARGUMENT  # one material short
    assert det.binding([0] + [tc.NO_TEXTURE] * (nm - 1)) == 0 and det.commit() == PT_ERR_INVALID_ARGUMENT  # texture 0 is not set
    assert b"not set" in det.N.lib.pt_last_error(None)
    assert det.texture(0, tc.distinct(2, 2)) == 0 and det.commit() == 0
    assert det.info(0)[1].materials == 1
    assert det.uvs(np.full((n, 6), np.nan, np.float32)) == PT_ERR_INVALID_ARGUMENT and det.commit() == 0  # the refused call changed nothing
    assert det.texture(0, None) == 0 and det.commit() == PT_ERR_INVALID_ARGUMENT  # removed while bound
    assert det.binding(None) == 0 and det.commit() == 0
    assert det.uvs(None) == 0 and det.commit() == 0
    # the blob does not depend on any of it
    info = det.N.pt_bvh_info()
    assert det.N.lib.pt_scene_bvh_info(det.s, C.byref(info)) == 0 and info.n_tris == n


def test_blob_is_the_same_with_and_without_textures(P):
    sd = P.make_scene(P.native.PT_SCENE_CORNELL_TESS, 400, 3, W, H)
    from pathtracing_amd.host import build_bvh_detached
    plain = build_bvh_detached(sd, 68)
    d = Detached(P)
    try:
        L, p = d.N.lib, lambda a: a.ctypes.data_as(C.c_void_p)
        v, tm = np.ascontiguousarray(sd.verts, np.float32), np.ascontiguousarray(sd.tri_mat, np.uint32)
        assert L.pt_scene_set_triangles(d.s, p(v), p(tm), len(tm)) == 0
        assert d.uvs(tc.random_uvs(len(tm))) == 0 and d.texture(2, tc.distinct(3, 5)) == 0 and d.binding([2] * len(sd.mats)) == 0
        assert L.pt_scene_commit(d.s, 68) == 0
        info = d.N.pt_bvh_info()
        assert L.pt_scene_bvh_info(d.s, C.byref(info)) == 0
        nodes, tris = np.zeros(int(info.node_bytes), np.uint8), np.zeros(int(info.tri_bytes), np.uint8)
        assert L.pt_scene_bvh_read(d.s, p(nodes), info.node_bytes, p(tris), info.tri_bytes) == 0
        assert np.array_equal(nodes, plain[1]) and np.array_equal(tris, plain[2])
    finally:
        d.close()


# ------------------------------------------------------------------------------------------------------------------------ pipeline.h
_BITS = [FLAGS[k] for k in ("PROFILE_KERNELS", "COUNT_VISITS", "EXTEND_PACKED", "EXTEND_SIMPLE", "BUCKET_SPECULAR", "SPLIT_KERNELS", "EXTEND_POOL",
                            "NEXT_EVENT")] + [512]  # 512: PT_FLAG_NEXT_EVENT_SPHERES


def _inputs():
    for n in range(len(_BITS) + 1):
        for combo in itertools.combinations(_BITS, n):
            for tuned, env, spec, lens, sphl in itertools.product(range(4), (0, 1), (0, 1), (0, 1), (0, 1)):
                yield sum(combo), tuned, env, spec, lens, sphl


def test_decode_with_textures_over_every_input(P):
    """has_textures = true: every refusal with its status and a message that names the rule, and what an accepted frame runs. The
    expectations restate docs/SPEC.md §13's "Where it runs" on their own."""
    N = P.native
    assert N.PT_FLAG_NEXT_EVENT_SPHERES == 512
    seen = {"textured": 0, "lens": 0, "sphere": 0, "ok": 0, "invalid": 0}
    for flags, tuned, env, spec, lens, sphl in _inputs():
        d = tc.decode(flags, tuned, env, spec, lens, sphl, textures=True)
        nee, spheres = bool(flags & FLAGS["NEXT_EVENT"]), bool(flags & 512)
        forced = 3 if flags & FLAGS["EXTEND_POOL"] else 2 if flags & FLAGS["EXTEND_PACKED"] else 1 if flags & FLAGS["EXTEND_SIMPLE"] else tuned
        other = bool(flags & (FLAGS["SPLIT_KERNELS"] | FLAGS["BUCKET_SPECULAR"])) or forced in (2, 3)
        ctx = (flags, tuned, env, spec, lens, sphl)
        if spheres and not nee:
            assert d.status == PT_ERR_INVALID_ARGUMENT, ctx
            seen["invalid"] += 1
        elif other or flags & FLAGS["COUNT_VISITS"]:
            assert d.status == PT_ERR_UNSUPPORTED and b"textured" in d.message and b"one-ray-per-lane" in d.message, ctx
            seen["textured"] += 1
        elif lens:
            assert d.status == PT_ERR_UNSUPPORTED and b"textured" in d.message and b"lens" in d.message, ctx
            seen["lens"] += 1
        elif spheres and sphl:
            assert d.status == PT_ERR_UNSUPPORTED and b"textured" in d.message and b"sphere light" in d.message, ctx
            seen["sphere"] += 1
        else:
            assert d.status == 0 and d.message is None, ctx
            assert (d.tex, d.forced, d.shade, d.fuse, d.full_state, d.count, d.split, d.lens, d.sph) == (1, 1, 2, 2, 0, 0, 0, 0, 0), ctx
            assert (d.nee, d.env) == (int(nee), env) and d.kernel_for[0][0] == d.kernel_for[1][0] == 1, ctx
            assert tc.extend_instantiated(1, d.fuse, d.count, d.nee, d.env, d.lens, d.sph, d.tex), ctx
            seen["ok"] += 1
    assert all(seen.values()), seen


def test_decode_without_textures_is_the_decode_without_the_argument():
    for args in _inputs():
        assert tc.decode(*args, textures=False).fields() == tc.decode(*args, textures=None).fields(), args


def test_textured_instantiations():
    """Four per layout: the one-ray-per-lane kernel, all-kinds fused shading, no counting, with and without NEE and the environment,
    neither through a lens nor with sphere lights. Without tex the table is the one it was."""
    n = 0
    for kernel, fuse, count, nee, env, lens, sph in itertools.product(range(0, 5), range(-2, 4), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1)):
        want = kernel == 1 and fuse == 2 and not count and not lens and not sph
        assert tc.extend_instantiated(kernel, fuse, count, nee, env, lens, sph, 1) == want, (kernel, fuse, count, nee, env, lens, sph)
        n += want
    assert n == 4


# ------------------------------------------------------------------------------------------------------------------------ the lookup
A, B, Cc, D = (np.array(v, np.float32) for v in ((0.125, 0.25, 0.5), (0.375, 0.75, 1.0), (0.625, 1.25, 1.5), (0.875, 0.5, 2.0)))
T22 = np.array([[A, B], [Cc, D]], np.float32)  # row 0 (t in [0, 1/2)): A B; row 1: C D. Eighths: every mean below is exact in f32.


def mean(*t):
    return (np.sum(np.array(t, np.float64), 0) / len(t)).astype(np.float32)


@pytest.mark.parametrize("s,t,want", [
    (0.25, 0.25, A), (0.75, 0.25, B), (0.25, 0.75, Cc), (0.75, 0.75, D),                       # the centres
    (0.5, 0.25, mean(A, B)), (0.5, 0.75, mean(Cc, D)), (0.25, 0.5, mean(A, Cc)), (0.75, 0.5, mean(B, D)),  # the midpoints inside
    (0.0, 0.25, mean(A, B)), (0.25, 0.0, mean(A, Cc)),                                         # ... and across the wrap
    (-0.25, 0.25, B), (0.25, -0.25, Cc), (-0.25, -0.25, D),                                    # -0.25 is 0.75
    (1.0, 0.25, mean(A, B)), (1.0, 1.0, mean(A, B, Cc, D)), (1.25, 2.25, A),                   # 1.0 is 0.0
    (1048576.0, 0.25, mean(A, B)), (-1048576.0, 0.75, mean(Cc, D)), (1048575.75, 0.25, B),     # 2^20 is 0.0, and 3 fraction bits are left
    (0.0, 0.0, mean(A, B, Cc, D)), (0.5, 0.5, mean(A, B, Cc, D)),                              # the wrap corner, and the middle
    (-1e-9, 0.25, mean(A, B)), (0.25, -1e-9, mean(A, Cc)), (-1e-9, -1e-9, mean(A, B, Cc, D)),  # s - floorf(s) == 1.0f: x0 = W - 1, x1 = 0
])
def test_bilinear_known_answers(s, t, want):
    got = tc.lookup(T22, s, t)
    assert np.array_equal(got, want), (s, t, got.tolist(), want.tolist())


@pytest.mark.parametrize("s,t,want", [
    (0.25, 0.25, A), (0.75, 0.25, B), (0.25, 0.75, Cc), (0.75, 0.75, D),
    (0.0, 0.0, A), (0.49999997, 0.5, Cc), (0.5, 0.49999997, B),                                # the texel the coordinate falls in
    (-0.25, 0.25, B), (1.0, 0.25, A), (1.0, 1.0, A), (1048576.0, -1048576.0, A), (1048575.75, 0.25, B),
    (-1e-9, 0.25, B), (0.25, -1e-9, Cc), (-1e-9, -1e-9, D),                                    # s - floorf(s) == 1.0f lands on the last texel
])
def test_nearest_known_answers(s, t, want):
    got = tc.lookup(T22, s, t, tc.NEAREST)
    assert np.array_equal(got, want), (s, t, got.tolist(), want.tolist())


def test_one_colour_and_one_texel_textures_are_exact():
    c = np.array([0.3, 0.7, 1.9], np.float32)
    rng = np.random.default_rng(3)
    for w, h in ((1, 1), (3, 5), (64, 64)):
        img = np.full((h, w, 3), c, np.float32)
        for s, t in (rng.random((200, 2)) * 9.0 - 4.0).astype(np.float32):
            for flags in (0, tc.NEAREST):
                assert np.array_equal(tc.lookup(img, s, t, flags), c), (w, h, s, t, flags)
    one = tc.distinct(1, 1)
    assert np.array_equal(tc.lookup(one, 0.3, -7.7), one[0, 0]) and np.array_equal(tc.lookup(one, -1e-9, 1.0, tc.NEAREST), one[0, 0])


def test_lookup_against_float64_on_odd_sizes():
    """3 x 5 distinct texels: the nearest texel is the float64 one away from texel borders, and the bilinear value is the float64
    interpolation of the four float64 neighbours within a few f32 roundings of the largest texel."""
    img = tc.distinct(3, 5)
    rng = np.random.default_rng(8)
    for s, t in (rng.random((300, 2)) * 6.0 - 3.0).astype(np.float32):
        fs, ft = float(s) - np.floor(float(s)), float(t) - np.floor(float(t))
        x, y = fs * 3, ft * 5
        if min(x % 1, 1 - x % 1, y % 1, 1 - y % 1) > 1e-4:
            assert np.array_equal(tc.lookup(img, s, t, tc.NEAREST), img[int(y), int(x)]), (s, t)
        xf, yf = x - 0.5, y - 0.5
        x0, y0 = int(np.floor(xf)), int(np.floor(yf))
        fx, fy = xf - x0, yf - y0
        p = img.astype(np.float64)
        want = ((1 - fy) * ((1 - fx) * p[y0 % 5, x0 % 3] + fx * p[y0 % 5, (x0 + 1) % 3])
                + fy * ((1 - fx) * p[(y0 + 1) % 5, x0 % 3] + fx * p[(y0 + 1) % 5, (x0 + 1) % 3]))
        # coordinate error: |s| <= 3 is rounded to 2^-22, times W or H <= 5 texels, times a texel difference <= 1; plus three lerps' roundings
        assert np.abs(tc.lookup(img, s, t) - want).max() <= 5 * 2.0 ** -22 + 6 * 2.0 ** -24 * 1.1, (s, t)


def test_coordinate_and_barycentrics():
    v9 = np.array([0, 0, -1, 2, 0, -1, 0, 2, -1], np.float32)
    u, v = tc.barycentrics(v9, (0.5, 0.25, 0.0), (0.0, 0.0, -1.0))
    assert (u, v) == (np.float32(0.25), np.float32(0.125))
    uv6 = np.array([0.0, 1.0, 8.0, 1.0, 0.0, 9.0], np.float32)
    assert tc.coordinate(uv6, u, v) == (np.float32(2.0), np.float32(2.0))
    assert tc.coordinate(uv6, 0.0, 0.0) == (np.float32(0.0), np.float32(1.0)) and tc.coordinate(uv6, 1.0, 0.0) == (np.float32(8.0), np.float32(1.0))


# ------------------------------------------------------------------------------------------------------------------------ the checker against the oracle
def params_of(P, **kw):
    return P.make_params(W, H, **kw)


@pytest.fixture(scope="module")
def oracle_frames(P, pto):
    """The oracle's untextured frames, computed once."""
    params = params_of(P, spp=4, max_depth=8, streams=2)
    out = {}
    for name in ("cornell", "glass", "soup"):
        sd = ec.scene(P, name, W, H)
        if name == "soup":
            sd = dataclasses.replace(sd, sky=np.ones(3, np.float32))  # its only light
        out[name] = (sd, pto.render(pto.Scene(sd), params))
    return params, out


@pytest.mark.parametrize("flags", [0, tc.NEAREST], ids=["bilinear", "nearest"])
@pytest.mark.parametrize("size", [(1, 1), (3, 5), (64, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_all_ones_texture_is_the_oracles_untextured_frame(P, pto, oracle_frames, size, flags):
    params, frames = oracle_frames
    ones = (np.ones((size[1], size[0], 3), np.float32), flags)
    for name in ("cornell", "glass", "soup"):
        sd, (want, ost) = frames[name]
        tsd = tc.textured(sd, {5: ones}, {m: 5 for m in range(len(sd.mats))}, uvs=tc.random_uvs(len(sd.verts)))
        got, st = tc.render(pto, pto.Scene(tsd), params, tsd)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, size, flags)
        assert st.ext_rays == ost.rays and st.paths == ost.paths and st.shadow_rays == 0, name


def test_untextured_checker_is_the_oracle_and_the_env_checker(P, pto, oracle_frames):
    """Without textures the checker is §5 (the oracle), and with PT_FLAG_NEXT_EVENT and an environment map it is tests/env_ref/, which its own
    tests hold to the oracle; all-ones textures change neither."""
    params, frames = oracle_frames
    sun = ec.sun_sky(P, 16)
    for name in ("cornell", "glass"):
        sd, (want, _) = frames[name]
        got, _ = tc.render(pto, pto.Scene(sd), params, None)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
        tsd = tc.textured(sd, {0: np.ones((3, 5, 3), np.float32)}, {m: 0 for m in range(len(sd.mats))})
        for env, nee in ((None, True), (sun, False), (sun, True)):
            ref, est, _ = ec.render(pto, pto.Scene(sd), params, env=env, flags=ec.NEE if nee else 0)
            for x in (None, tsd):
                got, st = tc.render(pto, pto.Scene(sd), params, x, env=env, nee=nee)
                assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (name, env is not None, nee, x is not None)
                assert (st.ext_rays, st.shadow_rays, st.paths) == (est.ext_rays, est.shadow_rays, est.paths)


@pytest.mark.parametrize("flags", [0, tc.NEAREST], ids=["bilinear", "nearest"])
def test_one_colour_texture_is_the_oracles_frame_with_the_product_albedo(P, pto, flags):
    """A texture of one colour c on the walls of the glass Cornell box (whose wall materials no sphere carries) and on the soup: the
    oracle's frame of the scene whose bound materials have the albedo fl(a * c)."""
    c = np.array([0.9, 0.5, 1.25], np.float32)
    params = params_of(P, spp=4, max_depth=8, streams=2)
    for name, bound in (("glass", (0, 1, 2)), ("soup", (0,))):
        sd = ec.scene(P, name, W, H)
        if name == "soup":
            sd = dataclasses.replace(sd, sky=np.ones(3, np.float32))  # its only light
        tsd = tc.textured(sd, {9: (np.full((5, 3, 3), c, np.float32), flags)}, {m: 9 for m in bound}, uvs=tc.random_uvs(len(sd.verts)))
        mats = sd.mats.copy()
        for m in bound:
            mats[m]["albedo"] = mats[m]["albedo"] * c  # one f32 multiply per component
        want, ost = pto.render(pto.Scene(dataclasses.replace(sd, mats=mats)), params)
        got, st = tc.render(pto, pto.Scene(tsd), params, tsd)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, flags)
        assert st.ext_rays == ost.rays
        plain, _ = pto.render(pto.Scene(sd), params)
        assert not np.array_equal(plain, want)  # the texture is seen


def test_a_bound_sphere_material_stays_plain_and_distinct_texels_show(P, pto):
    """C1's white material is on three walls and two spheres. Bound to a black texture, the walls turn black while the white spheres
    still reflect: the frame is not the one with a black albedo, but the one in which only the walls' copy of the material is black."""
    sd = ec.scene(P, "cornell", W, H)
    params = params_of(P, spp=2, max_depth=4, streams=1)
    tsd = tc.textured(sd, {0: np.zeros((2, 2, 3), np.float32)}, {0: 0})
    got, _ = tc.render(pto, pto.Scene(tsd), params, tsd)
    mats = sd.mats.copy()
    mats[0]["albedo"] = 0
    black, _ = pto.render(pto.Scene(dataclasses.replace(sd, mats=mats)), params)
    assert not np.array_equal(got, black)
    # the same with the spheres given a white material of their own is the oracle's frame
    m2 = np.concatenate([mats, sd.mats[:1]])
    sm = np.where(sd.sph_mat == 0, len(sd.mats), sd.sph_mat).astype(np.uint32)
    want, _ = pto.render(pto.Scene(dataclasses.replace(sd, mats=m2, sph_mat=sm)), params)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # distinct texels: a textured frame is neither the plain one nor flat
    d = tc.cornell(P, W, H, tc.distinct(3, 5), (tc.distinct(2, 2, 40), tc.NEAREST))
    img, _ = tc.render(pto, pto.Scene(d), params, d)
    plain, _ = pto.render(pto.Scene(sd), params)
    assert not np.array_equal(img, plain) and np.isfinite(img).all()


def test_texture_from_srgb8(P):
    img = np.array([[[0, 255, 128, 7], [10, 11, 188, 9]]], np.uint8)
    lin = P.texture_from_srgb8(img)
    assert lin.shape == (1, 2, 3) and lin.dtype == np.float32
    assert lin[0, 0, 0] == 0.0 and lin[0, 0, 1] == 1.0 and abs(lin[0, 0, 2] - 0.2158605) < 1e-6 and abs(lin[0, 1, 0] - 10 / 255 / 12.92) < 1e-7
    with pytest.raises(ValueError):
        P.texture_from_srgb8(np.zeros((2, 2, 3), np.float32))
