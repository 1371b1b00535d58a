"""-m gpu: the device's BSDFs and path loop on the material zoo (tests/material_zoo.py), bit for bit against the oracle on the device's
own BVH bytes: every zoo scene and camera on three layouts and all six shading pipelines (fused one-ray-per-lane, lane-packing,
pooled, split k_shade, bucketed specular, and the probed default), the depth and roulette edges, progressive frames, next-event
estimation with lights of every material kind, and the denoiser's guides. tests/test_materials.py (CPU) shows with a branch census
that these very frames reach every branch of docs/SPEC.md §5's samplers; only scenes that pass it are rendered here."""
import numpy as np
import pytest

import denoise_checker as dc
import material_zoo as mz
from frame_checks import check_denoise, check_nee, run_both
from material_zoo import NEE_CONFIGS, emissive_triangles
from pipelines import named_flags

pytestmark = pytest.mark.gpu

ZOO_LAYOUTS = [0, 68, 73]


def pipelines(P):
    return named_flags("probed", "simple", "packed", "pool", "split", "bucket")


def equal_to_the_oracle(P, pto, r, sd, params, layout, count, ctx):
    """Frame, rays and paths (and with `count` the visit counters) of the device equal the oracle's on the device's own blob."""
    img, st, ref, ost = run_both(P, pto, r, sd, params, layout, count=count)
    assert np.isfinite(img).all(), ctx
    bad = np.argwhere((img != ref).any(axis=2))
    assert np.array_equal(img, ref), (ctx, len(bad), bad[:4].tolist(), img[tuple(bad[0])].tolist(), ref[tuple(bad[0])].tolist())
    assert (st.rays, st.paths) == (ost.rays, ost.paths), (ctx, st.rays, ost.rays)
    if count:
        assert (st.node_visits, st.tri_tests, st.sphere_tests) == (ost.node_visits, ost.tri_tests, ost.sphere_tests), ctx
    return st


@pytest.mark.parametrize("layout", ZOO_LAYOUTS)
@pytest.mark.parametrize("cfg", mz.CONFIGS, ids=["-".join(c) for c in mz.CONFIGS])
def test_parity_on_every_pipeline(P, pto, renderer, cfg, layout):
    sd = mz.build(*cfg)
    pair = mz.CONFIGS.index(cfg) * len(ZOO_LAYOUTS) + ZOO_LAYOUTS.index(layout)
    for i, (name, flags) in enumerate(pipelines(P)):  # visit counters on every second case: each pipeline on half of the pairs
        equal_to_the_oracle(P, pto, renderer, sd, mz.parity_params(P, flags), layout, (pair + i) % 2 == 1, (cfg, layout, name))


@pytest.mark.parametrize("key", list(mz.EDGE_PARAMS))
@pytest.mark.parametrize("cfg", mz.EDGE_SCENES, ids=["-".join(c) for c in mz.EDGE_SCENES])
def test_depth_and_roulette_edges(P, pto, renderer, cfg, key):
    """max_depth 1, 2 and 255, Russian roulette from the first vertex and never, fewer samples than streams."""
    N = P.native
    sd = mz.build(*cfg)
    for name, flags in named_flags("probed", "pool", "bucket"):
        st = equal_to_the_oracle(P, pto, renderer, sd, mz.edge_params(P, key, flags), 0, False, (cfg, key, name))
        if key == "depth1":
            assert st.rays == mz.W * mz.H * 4


def test_progressive_frames(P, pto, renderer):
    """3 + 2 samples with PT_FLAG_ACCUMULATE on the palette are the oracle's 5-sample frame."""
    N = P.native
    sd = mz.build("palette", "front")
    renderer.SetScene(sd, 0)
    done = 0
    for n in (3, 2):
        renderer.Params = P.make_params(mz.W, mz.H, spp=n, max_depth=12, streams=2, sample_offset=done,
                                        flags=N.PT_FLAG_ACCUMULATE if done else 0)
        renderer.Render(0.0)
        done += n
    img = renderer.ReadFramebuffer()
    osc = pto.Scene(sd, (renderer.BvhInfo().width,) + renderer.BvhRead())
    ref, _ = pto.render(osc, P.make_params(mz.W, mz.H, spp=5, max_depth=12, streams=2))
    assert np.isfinite(img).all() and np.array_equal(img, ref)


@pytest.mark.parametrize("cfg", NEE_CONFIGS, ids="-".join)
def test_next_event_estimation(P, pto, renderer, cfg):
    """PT_FLAG_NEXT_EVENT against the scalar checker of SPEC §7, bit for bit; rays = extension + shadow rays; the light set is every
    emissive triangle of positive area, whatever its material kind."""
    sd = mz.build(*cfg)
    lit = emissive_triangles(sd)
    if cfg[0] == "palette":
        assert {int(k) for k in sd.mats["kind"][sd.tri_mat[lit]]} == {0, 1, 2}
    for layout in ZOO_LAYOUTS:
        renderer.SetScene(sd, layout)
        params = mz.parity_params(P, P.native.PT_FLAG_NEXT_EVENT)
        renderer.Params = params
        st, cst = check_nee(P, pto, renderer, sd, params, (cfg, layout))
        assert cst.n_lights == int(lit.sum()) > 0 and cst.shadow_rays > 0


def test_guides_of_every_material(P, pto, renderer):
    """pt_denoise's guides on the palette: normal, depth, the albedo of every material hit and the primitive id, bit for bit."""
    sd = mz.build("palette", "front")
    for layout in ZOO_LAYOUTS:
        renderer.SetScene(sd, layout)
        renderer.Params = mz.parity_params(P)
        renderer.Render(0.0)
        _, g, _ = check_denoise(P, pto, renderer, sd, ("palette", layout), guides_only=True)
        ids = g[..., 7].view(np.uint32)
        hit = ids != dc.MISS
        mats = np.concatenate([sd.tri_mat, sd.sph_mat])[ids[hit]]
        assert np.array_equal(g[..., 4:7][hit], sd.mats["albedo"][mats])       # g1's albedo is the hit material's, whatever its kind
        assert len(np.unique(mats)) >= 40 and {int(k) for k in sd.mats["kind"][mats]} == {0, 1, 2} and mats.max() >= 300
        assert np.isfinite(g[..., :7][hit]).all()
