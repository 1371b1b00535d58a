"""-m gpu: the texture lookup (docs/SPEC.md §13, texture_device.h's tex_of_hit) on the device across the texture and UV space
(tests/texture_space.py has the cases and the probe scene; tests/test_texture_space.py holds the scalar checker to the float64
reference of tests/tex64.py on them without a device).

Both consumers of tex_of_hit are held, on 48 x 36 probes of the tile wall:

* the guides (k_guide_resolve_tex): g1.rgb / albedo at TraceRays' (u, v) of the guide rays;
* frames (shade_one<TEX> in k_extend): a sky of exactly 1, max_depth 2, one sample — a wall pixel is albedo * texel exactly.

Each against float64 by texture_space.hold (tol at near points, candidates for the nearest filter, the envelope, finiteness, a one-colour
texture's colour) and against the scalar checker bit for bit, for every size x filter x contents of a family; over layouts and both
builders; on a contact sheet of 64 textures of which 40 are bound; and through replaced textures, rebound materials and moved
geometry on one context, against a fresh SetScene of the same scene."""
import dataclasses

import numpy as np
import pytest

import ray_caster64 as rc
import texture_space as ts

pytestmark = pytest.mark.gpu

W, H = ts.W, ts.H
LBVH = 0x100


@pytest.fixture(scope="module")
def rays(P, pto):
    """The probe camera's jitter-free rays."""
    assert P.native.PT_BVH_BUILD_LBVH == LBVH
    return rc.camera_rays(pto, ts.probe((1, 1), "distinct", "unit", 0).scene(P).cam, W, H)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def look(P, r, rays):
    """What both consumers looked up on the renderer's current scene: (ids, u, v of the pixels that hit the wall, their pixel
    indices, the guides' texels, the frame's texels) — g1.rgb and the frame's rgb over the albedo, a power of two."""
    r.Params = P.make_params(W, H, spp=1, max_depth=2, rr_start=8, streams=1)
    st = r.Render(0.0)
    assert st.reserved[0] == 1
    frame = r.ReadFramebuffer()[..., :3].reshape(-1, 3)
    assert r.Denoise(iterations=1).rays == W * H
    g = r.ReadGuides().reshape(-1, 8)
    hits, _ = r.TraceRays(rays)
    ids = np.ascontiguousarray(hits[:, 1]).view(np.uint32)
    assert np.array_equal(ids, np.ascontiguousarray(g[:, 7]).view(np.uint32))
    px = np.nonzero(ids != ts.MISS)[0]
    assert len(px) >= 0.95 * W * H and (ids[px] < ts.N_TRIS).all()
    assert (np.delete(frame, px, axis=0) == 1.0).all()  # the sky
    scale = np.float32(1.0 / ts.ALBEDO)
    return ids[px].astype(np.int64), hits[px, 2].copy(), hits[px, 3].copy(), px, g[px, 4:7] * scale, frame[px] * scale


def judge(sheet, seen, ctx):
    """Guides and frame of `seen` = look(..) against the scalar checker bit for bit and against float64 by texture_space.hold."""
    ids, u, v, px, guide, frame = seen
    want = ts.checker_texels(sheet, ids, u, v)
    for name, got in (("guides", guide), ("frame", frame)):
        bad = np.nonzero((bits(got) != bits(want)).any(1))[0]
        assert len(bad) == 0, (ctx, name, "differs from the checker", len(bad), px[bad[:4]].tolist(), got[bad[0]].tolist(), want[bad[0]].tolist())
    res = ts.hold(sheet, ids, u, v, guide, (ctx, "guides"))
    ts.hold(sheet, ids, u, v, frame, (ctx, "frame"))
    return res


@pytest.mark.parametrize("family", ts.FAMILIES)
def test_guides_and_frames_across_the_space(P, renderer, rays, family):
    """Every size x filter x contents of the family, the subject between its guards. The FLT_MAX texel stays in: with the albedo 0.5
    and one sample no sum of the frame path leaves f32's range."""
    for size in ts.SIZES:
        worst = 0.0
        for contents in ts.CONTENTS:
            for name, flags in ts.FILTERS.items():
                sheet = ts.probe(size, contents, family, flags)
                renderer.SetScene(sheet.scene(P), 0)
                res = judge(sheet, look(P, renderer, rays), (family, size, contents, name))
                worst = max(worst, res[ts.SUBJECT][0])
                if name == "bilinear" and family != "constants" and ts.stated(size, contents, family) == "near":
                    assert res[ts.SUBJECT][1] == res[ts.SUBJECT][2], (family, size, contents, "a near case with far points", res[ts.SUBJECT])
        print(f"device {family} {size[0]}x{size[1]}: largest err / tol {worst:.3f}")


def test_layouts_and_builders(P, renderer, rays):
    """sheared on 63 x 65 over layouts {2, 68} x {default, PT_BVH_BUILD_LBVH}: the same bits from all four."""
    for name, flags in ts.FILTERS.items():
        sheet = ts.probe((63, 65), "distinct", "sheared", flags)
        first = None
        for layout in (2, 68, 2 | LBVH, 68 | LBVH):
            renderer.SetScene(sheet.scene(P), layout)
            seen = look(P, renderer, rays)
            judge(sheet, seen, ("sheared", name, layout))
            if first is None:
                first = seen
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(first, seen)), (name, layout)


def check_info(r, sheet):
    """pt_scene_texture_info: W H 16 device bytes for a bound texture, none for one that is only set."""
    for i, T in sheet.textures.items():
        info = r.TextureInfo(i)
        n = int((sheet.tile_texture == i).sum())
        assert (info.width, info.height, info.flags, info.materials) == (T.size[0], T.size[1], T.flags, n), i
        assert info.device_bytes == (T.size[0] * T.size[1] * 16 if n else 0), (i, info.device_bytes)


def test_contact_sheet(P, renderer, rays):
    """64 textures of different sizes and disjoint values set, 40 bound, unbound ones below, between and above them: every pixel is its
    own tile's texture."""
    sheet = ts.contact_sheet()
    assert len(set(T.size for T in sheet.textures.values())) == 64 and len(np.unique(sheet.tile_texture)) == 40
    unbound = sorted(set(range(64)) - set(ts.CONTACT_BOUND))
    assert unbound[0] == 0 and unbound[-1] == 63 and any(ts.CONTACT_BOUND[0] < i < ts.CONTACT_BOUND[-1] for i in unbound)
    renderer.SetScene(sheet.scene(P), 0)
    res = judge(sheet, look(P, renderer, rays), "contact sheet")
    assert sorted(res) == ts.CONTACT_BOUND  # every bound texture was seen
    assert all(n_near == n for k, (_, n_near, n) in res.items() if not sheet.textures[k].flags and sheet.textures[k].size != (1, 1)), res
    check_info(renderer, sheet)


def test_reuse_on_one_context(P, renderer, rays):
    """On a context of its own: the contact sheet; texture 1 replaced by a larger one, then by a 1 x 1; half the materials rebound; then,
    committed with the LBVH builder in layout 68, the wall moved by UpdateGeometry. After each step the guides and the frame are those of
    a fresh SetScene of the same scene on another context, bit for bit, and hold against float64."""
    sheet = ts.contact_sheet()
    r = P.Renderer(P.Window(W, H))
    r.Init()
    try:
        def step(ctx, layout=0):
            seen = look(P, r, rays)
            judge(sheet, seen, ctx)
            check_info(r, sheet)
            renderer.SetScene(sheet.scene(P), layout)
            fresh = look(P, renderer, rays)
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(seen, fresh)), (ctx, "differs from a fresh scene")

        r.SetScene(sheet.scene(P), 0)
        step("committed")
        for size in ((200, 150), (1, 1)):
            T = ts.contact_texture(1, size)
            sheet = dataclasses.replace(sheet, textures={**sheet.textures, 1: T})
            r.SetTexture(1, T.img, T.flags)
            r.Commit(0)
            step(("texture 1 replaced", size))
        tt = sheet.tile_texture.copy()
        tt[::2] = np.array(ts.CONTACT_BOUND)[(np.arange(ts.N_TILES)[::2] + 7) % len(ts.CONTACT_BOUND)]
        sheet = dataclasses.replace(sheet, tile_texture=tt)
        r.SetMaterialTextures(tt.astype(np.uint32))
        r.Commit(0)
        step("half the materials rebound")
        r.Commit(68 | LBVH)
        step("committed again, LBVH", 68 | LBVH)
        sheet = dataclasses.replace(sheet, verts=ts.sheared_verts())
        r.UpdateGeometry(verts=sheet.verts)
        step("moved", 68 | LBVH)
    finally:
        r.Dispose()
