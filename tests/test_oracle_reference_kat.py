"""The oracle's restatement of the reference's only ray kernel (Test.hlsl:1-40) against the known-answer
table of SURVEY.md §8c. This is the one part of the path the reference pins."""
import numpy as np

from reference_kat import KAT, check_against_kat


def test_reference_sphere_kat(pto):
    f, b = pto.reference_sphere(KAT["width"], KAT["height"])
    check_against_kat(f, b)


def test_unorm8_quantisation(pto):
    # R8G8B8A8Unorm store (Renderer.cs:124): clamp, scale, round
    cases = {-1.0: 0, 0.0: 0, 1.0: 255, 2.5: 255, 0.5: 128, 0.4980392: 127, float("nan"): 0, 1e-9: 0, 0.00197: 1}
    for v, want in cases.items():
        assert pto.lib.pto_unorm8(v) == want, v


def test_reference_sphere_small_frames(pto):
    # any W x H is the top-left crop of the 1920x1080 frame: uv depends on the pixel index only (Test.hlsl:6-7)
    full, full8 = pto.reference_sphere(640, 360)
    part, part8 = pto.reference_sphere(100, 37)
    assert np.array_equal(full[:37, :100], part) and np.array_equal(full8[:37, :100], part8)
