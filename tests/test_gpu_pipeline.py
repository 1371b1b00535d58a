"""-m gpu: pt_render against the device-free decode of its pipeline (tests/pipeline_checker.py over pathtracing_amd/csrc/pipeline.h) on
every combination of the eight flags that choose or narrow the pipeline, without and with an environment map: 2 x 256 frames of 16 x 16
pixels. The library refuses exactly the rows the decode refuses, with its status and message; every other frame is finite, and a forced
kernel is the one pt_stats.reserved[0] reports. What the frames hold is the parity tests' business (test_gpu_parity.py and the others
that select from tests/pipelines.py)."""
import dataclasses
import itertools

import numpy as np
import pytest

import pipeline_checker as pc
import pipelines as pl

pytestmark = pytest.mark.gpu

W = H = 16
BITS = [pl.FLAGS[n] for n in ("PROFILE_KERNELS", "COUNT_VISITS", "EXTEND_PACKED", "EXTEND_SIMPLE", "BUCKET_SPECULAR", "SPLIT_KERNELS",
                              "EXTEND_POOL", "NEXT_EVENT")]


def test_render_refuses_and_runs_what_the_decode_says(P, renderer):
    N = P.native
    # Cornell box with a glass and a metal sphere: an emissive triangle pair (NEE has a light) and specular materials (all-kinds shading)
    sd = P.make_scene(N.PT_SCENE_CORNELL_GLASS, 0, 3, W, H)
    sky = np.full((4, 4, 3), 0.25, np.float32)
    sky[1, 2] = (4.0, 3.0, 2.0)
    by_name = {p.flags: p for p in pl.RUNNABLE}
    tuned = renderer.GetTuning().extend_kernel
    renderer.SetTuning(extend_kernel=0)
    try:
        seen = {"refused": 0, "accepted": 0}
        for env in (None, sky):
            renderer.SetScene(dataclasses.replace(sd, environment=env), 0)
            for bits in itertools.product((0, 1), repeat=len(BITS)):
                flags = sum(b for b, on in zip(BITS, bits) if on)
                d, ctx = pc.decode(flags, 0, env is not None, True), (flags, env is not None)
                renderer.Params = P.make_params(W, H, spp=2, max_depth=4, streams=1, flags=flags)
                if d.status != 0:
                    seen["refused"] += 1
                    with pytest.raises(P.PtException) as e:
                        renderer.Render(0.0)
                    assert e.value.status == d.status == N.PT_ERR_UNSUPPORTED, ctx
                    assert str(e.value) == f"ptrt status {d.status}: {d.message.decode()}", ctx
                    continue
                seen["accepted"] += 1
                st = renderer.Render(0.0)
                assert np.isfinite(renderer.ReadFramebuffer()).all(), ctx
                if d.forced:
                    assert st.reserved[0] == d.forced, (ctx, st.reserved[0], d.forced)
                if env is None and flags in by_name and by_name[flags].kernel:
                    assert st.reserved[0] == by_name[flags].kernel, (ctx, by_name[flags].name)
        # accepted without a map: the 128 rows without NEE, and of NEE's the 4 that leave PROFILE_KERNELS and EXTEND_SIMPLE free;
        # with one: the 8 that leave those two and NEXT_EVENT free
        assert seen == {"refused": 124 + 248, "accepted": 132 + 8}, seen
    finally:
        renderer.SetTuning(extend_kernel=tuned)
