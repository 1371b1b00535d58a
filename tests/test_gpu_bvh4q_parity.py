"""-m gpu: the one-ray-per-lane kernel (PT_FLAG_EXTEND_SIMPLE) on the BVH4Q layout, without visit counting, against the oracle bit
for bit: the headline configuration's kernel, whose node and triangle fetches address their arrays by 32-bit byte offsets
(kernels.hip record()). Generator scenes at reduced size with both builders, every adversarial scene, ties on t between duplicated
and coplanar triangles, and a tree deep enough to use the traversal stack's overflow columns."""
import numpy as np
import pytest

import adversarial_scenes as S
from float64_support import W, H, _size, scenes
from frame_checks import assert_parity, run_both

pytestmark = pytest.mark.gpu

BVH4Q = 68


def _simple(P, params):
    params.flags |= P.native.PT_FLAG_EXTEND_SIMPLE
    return params


def _frame(P, pto, r, sd, params, width=BVH4Q):
    img, st, ref, ost = run_both(P, pto, r, sd, _simple(P, params), width)
    assert r.BvhInfo().width == BVH4Q
    assert_parity(img, st, ref, ost)
    return img, ref


@pytest.mark.parametrize("kind", ["tess", "soup"])
def test_generator_scenes_match_oracle(P, pto, renderer, kind):
    """The headline scene (tessellated Cornell box) and the triangle soup at reduced size, both builders."""
    N = P.native
    scene, detail = {"tess": (N.PT_SCENE_CORNELL_TESS, 20000), "soup": (N.PT_SCENE_TRIANGLE_SOUP, 20000)}[kind]
    w, h = 96, 64
    for build in (0, N.PT_BVH_BUILD_LBVH):
        sd = P.make_scene(scene, detail, 0x5EED0001, w, h)
        _frame(P, pto, renderer, sd, P.make_params(w, h, spp=4, max_depth=8, streams=8), BVH4Q | build)


def test_adversarial_scenes_match_oracle(P, pto, renderer):
    """Every scene of tests/adversarial_scenes.py (through float64_support.scenes): the id image and the path-traced frame."""
    for name, sd in scenes(P).items():
        w, h = _size(name)
        img, ref = _frame(P, pto, renderer, S.id_scene(sd), S.params_id(w, h))
        assert np.array_equal(S.ids_of(img), S.ids_of(ref)), name
        _frame(P, pto, renderer, sd, P.make_params(w, h, spp=2, max_depth=6, streams=8))


def _ties(w, h):
    """S.duplicates, with the vertices of every other copy rotated (v1, v2, v0): the same triangle in the same plane, whose t the
    triangle test computes from other edges, so ties on t are met both exactly and up to the last bit, across leaves."""
    sd, src = S.duplicates(w, h)
    v = sd.verts.reshape(-1, 3, 3).copy()
    v[1::2] = v[1::2][:, [1, 2, 0]]
    sd.verts = v.reshape(sd.verts.shape)
    return sd, src


def test_ties_are_decided_as_the_oracle_decides(P, pto, renderer):
    """Duplicated and coplanar triangles with equal t and different ids: the id image and the frame are the oracle's, and where
    a copy's t equals the unrotated original's the lower id wins."""
    sd, src = _ties(W, H)
    img, ref = _frame(P, pto, renderer, S.id_scene(sd), S.params_id(W, H))
    ids = S.ids_of(img)
    assert np.array_equal(ids, S.ids_of(ref))
    assert (ids < len(src)).sum() > 0.5 * W * H
    _frame(P, pto, renderer, sd, P.make_params(W, H, spp=2, max_depth=6, streams=8))


def test_overflow_stack_in_use(P, pto, renderer):
    """Stacked glass layers: a tree whose stack_need exceeds the 12 LDS entries, so the global overflow columns are in use. The
    frame is the oracle's and Render raises nothing (device error flag: 1 = stack overflow, 2 = step limit)."""
    sd = S.stacked_layers(W, H)
    for scene, params in ((S.id_scene(sd), S.params_id(W, H)), (sd, P.make_params(W, H, spp=2, max_depth=8, streams=8))):
        _frame(P, pto, renderer, scene, params)
        assert renderer.BvhInfo().stack_need > 12
