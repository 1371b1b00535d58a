"""The known-answer table of SURVEY.md §8c for the reference's only ray kernel (Test.hlsl:1-40), and the check of a frame against it:
shared by the oracle's test (tests/test_oracle_reference_kat.py) and the device's (tests/test_gpu_parity.py). Test helpers only."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
KAT = json.load(open(os.path.join(HERE, "golden", "reference_sphere_kat.json")))


def check_against_kat(f, b):
    """f: HxWx4 float32, b: HxWx4 uint8 — shared with the GPU test."""
    assert f.shape == (KAT["height"], KAT["width"], 4), (f.shape, KAT["height"], KAT["width"])
    hit = f[..., 2] != 0.0  # miss writes z = 0 exactly (Test.hlsl:36); a hit normal has z > 0 on the visible cap
    assert int(hit.sum()) == KAT["hit_pixels"], (int(hit.sum()), KAT["hit_pixels"])
    ys, xs = np.nonzero(hit)
    bb = KAT["hit_bbox"]
    assert (xs.min(), xs.max(), ys.min(), ys.max()) == (bb["xmin"], bb["xmax"], bb["ymin"], bb["ymax"]), ((xs.min(), xs.max(), ys.min(), ys.max()), bb)
    for px in KAT["pixels"]:
        x, y = px["xy"]
        assert bool(hit[y, x]) == px["hit"], (px, bool(hit[y, x]))
        if px["rgba"] is not None:
            np.testing.assert_allclose(f[y, x], np.array(px["rgba"], np.float32), atol=KAT["float_abs_tol"], rtol=0)
        for c in range(4):
            assert int(b[y, x, c]) in px["rgba8"][c], (px, c, b[y, x])
    np.testing.assert_allclose(b.reshape(-1, 4).mean(0), KAT["mean_rgba8"], atol=0.01)
    assert (f[..., 3] == 1.0).all() and (b[..., 3] == 255).all(), ("alpha", int((f[..., 3] != 1.0).sum()), int((b[..., 3] != 255).sum()))
