"""Whole-frame checks that more than one GPU test module applies: the device against the oracle on the same blob (run_both,
assert_parity, check_against_oracle), against the NEE checker (check_nee) and the denoise checker (check_denoise), and the grid of
layout, builder and extend-kernel configurations such frames are taken on. Test helpers only.

Pytest rewrites `assert` only in test modules, so every assert here carries its own message."""
import numpy as np
import pytest

import denoise_checker as dc
import nee_checker as nc
import ray_caster64 as rc
from blob_scenes import blob
from pipelines import flags_of
from trace_support import H, LAYOUTS, MISS, W, ids_of, oracle, records

RMSE_TOL = 1e-4  # BASELINE.json north_star: "images within 1e-4 RMSE of the CPU reference"


def rmse(a, b):
    return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)) ** 2)))


def run_both(P, pto, r, sd, params, width=4, count=False):
    r.SetScene(sd, width)
    r.Params = params
    if count:
        r.Params.flags |= P.native.PT_FLAG_COUNT_VISITS
    st = r.Render(0.0)
    img = r.ReadFramebuffer()
    info = r.BvhInfo()
    osc = pto.Scene(sd, (info.width,) + r.BvhRead())
    assert osc.validate_bvh()[0] == 0, ("validate_bvh", osc.validate_bvh()[0], width)
    ref, ost = pto.render(osc, params)
    return img, st, ref, ost


def assert_parity(img, st, ref, ost, exact=True):
    assert st.rays == ost.rays, (st.rays, ost.rays)
    assert st.paths == ost.paths, (st.paths, ost.paths)
    e = rmse(img, ref)
    nbad = int((img != ref).any(axis=-1).sum())
    assert e <= RMSE_TOL, (e, nbad)
    assert np.array_equal(img[..., 3], ref[..., 3]), ("alpha", int((img[..., 3] != ref[..., 3]).sum()))
    if exact:
        assert nbad == 0, f"{nbad} pixels differ, rmse {e}"


def nee_params(P, **kw):
    p = P.make_params(W, H, **kw)
    p.flags |= P.native.PT_FLAG_NEXT_EVENT
    return p


def check_nee(P, pto, r, sd, params, ctx):
    """The device's NEE frame equals the checker's bit for bit; rays = extension + shadow rays; the extension rays are the plain
    frame's rays."""
    st = r.Render(0.0)
    img = r.ReadFramebuffer()
    ref, cst, _ = nc.render(pto, pto.Scene(sd), params)
    assert np.isfinite(img).all(), ctx
    bad = np.argwhere((img != ref).any(axis=2))
    assert len(bad) == 0, (ctx, len(bad), bad[:4].tolist(), img[tuple(bad[0])].tolist() if len(bad) else None,
                           ref[tuple(bad[0])].tolist() if len(bad) else None)
    assert st.rays == cst.ext_rays + cst.shadow_rays, (ctx, st.rays, cst.ext_rays, cst.shadow_rays)
    assert st.paths == cst.paths, (ctx, st.paths, cst.paths)
    return st, cst


def check_denoise(P, pto, r, sd, ctx, p=None, **kw):
    """Denoise the renderer's current frame; its guides and image equal the checker's bit for bit."""
    h, w = r.Params.height, r.Params.width
    st = r.Denoise(**kw)
    g = r.ReadGuides()
    want_g = dc.guides(pto, pto.Scene(sd), w, h)
    bad = np.argwhere((g.view(np.uint32) != want_g.view(np.uint32)).any(axis=2))
    assert len(bad) == 0, (ctx, len(bad), bad[:3].tolist(), g[tuple(bad[0])].tolist() if len(bad) else None,
                           want_g[tuple(bad[0])].tolist() if len(bad) else None)
    assert st.rays == w * h, (ctx, st.rays, w * h)
    p = p if p is not None else dc.params(kw.get("iterations", 0), kw.get("sigma_color", 0.0), kw.get("sigma_normal", 0.0),
                                          kw.get("sigma_depth", 0.0), kw.get("sigma_albedo", 0.0),
                                          (dc.GUIDES_ONLY if kw.get("guides_only") else 0) | (0 if kw.get("edge_stops", True) else dc.NO_EDGE_STOPS))
    if p.flags & dc.GUIDES_ONLY:
        with pytest.raises(P.PtException) as e:
            r.ReadDenoised()
        assert e.value.status == P.native.PT_ERR_NOT_COMMITTED, (ctx, e.value.status, P.native.PT_ERR_NOT_COMMITTED)
        return st, g, None
    img = r.ReadDenoised()
    want = dc.filter(r.ReadFramebuffer(), want_g, p)
    bad = np.argwhere((img.view(np.uint32) != want.view(np.uint32)).any(axis=2))
    assert len(bad) == 0, (ctx, len(bad), bad[:3].tolist(), img[tuple(bad[0])].tolist() if len(bad) else None,
                           want[tuple(bad[0])].tolist() if len(bad) else None)
    return st, g, img


def check_against_oracle(P, pto, r, sd, ctx, params=None):
    """The renderer's current blob validates against sd's vertices, renders the oracle's frame bit for bit (rays and paths too), and
    its closest-hit queries with visit counters equal pto_closest's."""
    info, nodes, tris = blob(r)
    osc = pto.Scene(sd, (info.width, nodes, tris))
    assert osc.validate_bvh()[0] == 0, ctx
    params = params or P.make_params(W, H, spp=2, max_depth=8, streams=2)
    r.Params = params
    st = r.Render(0.0)
    ref, ost = pto.render(osc, params)
    assert np.array_equal(r.ReadFramebuffer(), ref), ctx
    assert (st.rays, st.paths) == (ost.rays, ost.paths), (ctx, st.rays, st.paths, ost.rays, ost.paths)
    o, d = rc.camera_rays(pto, sd.cam, W, H)
    sel = slice(None, None, 3)
    o, d = o[sel], d[sel]
    ids, ts, ost = oracle(pto, osc, o, d)
    hits, qst = r.TraceRays(records(o, d), count_visits=True)
    assert np.array_equal(ids_of(hits), ids), ctx
    hit = ids != MISS
    assert np.array_equal(hits[hit, 0].view(np.uint32), ts[hit].view(np.uint32)), ctx
    assert (qst.node_visits, qst.tri_tests, qst.sphere_tests) == (ost.node_visits, ost.tri_tests, ost.sphere_tests), ctx
    return osc


def _config_grid(P):
    """12 (layout | builder, extend flags, count) configurations: every extend kernel in both its counting and its plain
    instantiation (6 x 2), with the layouts cycling underneath them and the builder switching after each pass over the
    five layouts, so every layout and both builders appear too."""
    N = P.native
    kernels = flags_of("probed", "simple", "packed", "pool", "split", "split+packed")
    out = []
    for i in range(2 * len(kernels)):
        width = LAYOUTS[i % len(LAYOUTS)] | (N.PT_BVH_BUILD_LBVH if (i // len(LAYOUTS)) % 2 else 0)
        out.append((width, kernels[i // 2], i % 2 == 0))
    return out
