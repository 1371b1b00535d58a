"""What the GPU tests of the thin lens share (tests/test_gpu_lens.py, tests/test_gpu_lens_space.py): the checker's frame, made once
per (scene, lens, split), and the comparison of the device's frame with it."""
import numpy as np

import lens_checker as lc

_refs = {}


def reference(P, pto, name, sd, lens, params):
    """The checker's frame of (scene `name` as `sd`, lens, params), computed once and shared."""
    key = (name, sd.cam.jitter, lens, params.spp, params.streams, params.sample_offset, params.flags & P.native.PT_FLAG_NEXT_EVENT)
    if key not in _refs:
        nee = bool(params.flags & P.native.PT_FLAG_NEXT_EVENT)
        _refs[key] = lc.render(pto, pto.Scene(sd), params, lens=lens, flags=lc.NEE if nee else 0)[:2]
    return _refs[key]


def check(P, pto, r, name, sd, lens, params, ctx):
    """The renderer's frame of its current scene and lens = the checker's, bit for bit; rays = extension + shadow rays."""
    st = r.Render(0.0)
    img = r.ReadFramebuffer()
    ref, cst = reference(P, pto, name, sd, lens, params)
    assert np.isfinite(img).all(), ctx
    bad = np.argwhere((img != ref).any(axis=2))
    assert len(bad) == 0, (ctx, len(bad), bad[:4].tolist(), img[tuple(bad[0])].tolist(), ref[tuple(bad[0])].tolist())
    assert st.rays == cst.ext_rays + cst.shadow_rays, (ctx, st.rays, cst.ext_rays, cst.shadow_rays)
    assert st.paths == cst.paths and st.reserved[0] == 1 and st.reserved[3] == 0, (ctx, st.paths, cst.paths, list(st.reserved))
    return st
