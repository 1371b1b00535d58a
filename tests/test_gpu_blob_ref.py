"""-m gpu: every byte of a committed or refitted blob against tests/blob_ref.py, the plain statement of what docs/SPEC.md §4.1 and §4.3
determine once the topology is fixed (tests/test_blob_ref.py holds that statement to the host builder and to hand-worked nodes without
a device).

The structural check only asks that boxes enclose, and the frame comparisons traverse the same blob on both sides, so boxes that are
too large, a grid exponent or an origin left over from the commit, or a refit that unites the new box with the stale one pass every
other test and only cost traversal speed. Here the node and record bytes are compared exactly, for the four producers: the device packer of
layout 68 (lbvh.hip), the host quantiser on a device-built tree and on the host's own, k_refit_tris and k_refit_level (refit.hip). The
only tolerance is one float32 step on the refit's sah_cost, derived in `check_sah`."""
import numpy as np
import pytest

import adversarial_scenes as S
import blob_ref as B
import lbvh_ref as L
from blob_scenes import NAMES, SCENES, blob, deform, moved
from blob_scenes import scene as lbvh_scene
from trace_support import LAYOUTS, scenes

pytestmark = pytest.mark.gpu

F = np.float32
REFIT_SCENES = SCENES + [n for n in ("random257", "random1025", "planar", "at_plus_1e4", "layers") if n not in SCENES]  # `layers` is in both
_update_scenes = {}


def get_scene(P, name):
    if name in SCENES:
        if not _update_scenes:
            _update_scenes.update(scenes(P))
        return _update_scenes[name]
    return lbvh_scene(P, name)[0]


def shrunk(sd):
    """Every triangle scaled by 1/4 about its own centroid."""
    v = np.asarray(sd.verts, F).reshape(-1, 3, 3).astype(np.float64)
    c = v.mean(axis=1, keepdims=True)
    return (c + 0.25 * (v - c)).astype(F).reshape(-1, 9)


def check_bytes(r, topo, sd, ctx):
    """The renderer's blob has the topology `topo` = (width, nodes, tris) — refs, id and material words — and every byte that
    blob_ref.expected_blob derives from that topology and sd's vertices. Returns (info, nodes, tris)."""
    info, nodes, tris = blob(r)
    width, tn, tt = topo
    assert info.width == width and nodes.size == tn.size and tris.size == tt.size, ctx
    assert np.array_equal(B.refs_of(width, nodes), B.refs_of(width, tn)), ctx
    w, tw = tris.view(np.uint32).reshape(-1, 12), tt.view(np.uint32).reshape(-1, 12)
    assert np.array_equal(w[:, 3], tw[:, 3]) and np.array_equal(w[:, 7], tw[:, 7]), ctx
    want = B.expected_blob(width, tn, tt, sd.verts, sd.tri_mat)
    assert B.blob_mismatches(width, nodes, tris, *want) == [], ctx
    return info, nodes, tris


def check_sah(info, topo, sd, ctx):
    """The refit's sah_cost is float32(exact_sah) within one float32 step. k_refit_sah adds the same non-negative float32 quotients
    f32(area / root area) (times a leaf's count) in double as exact_sah does; a double sum of n <= 1e7 such terms differs from the sum
    in any other order by less than n * 2^-53 < 1e-9 relative, far below half a float32 step (6e-8), so the two roundings to float32
    are the same float or neighbours."""
    want = F(B.sah_expected(topo[0], topo[1], topo[2], sd.verts))
    got = F(info.sah_cost)
    assert np.nextafter(want, F(-np.inf)) <= got <= np.nextafter(want, F(np.inf)), (ctx, float(got), float(want))


@pytest.mark.parametrize("name", NAMES)
def test_gpu_builder_blob_is_the_expected_blob(P, renderer, name):
    """PT_BVH_BUILD_LBVH on every layout: layout 68 is packed and quantised on the device (k_finalize), the others by the host packer
    from the device-built tree. Nodes and records equal expected_blob of the blob's own topology and the scene's vertices."""
    sd = lbvh_scene(P, name)[0]
    for layout in LAYOUTS:
        renderer.SetScene(sd, layout | P.native.PT_BVH_BUILD_LBVH)
        info, nodes, tris = blob(renderer)
        check_bytes(renderer, (info.width, nodes, tris), sd, (name, layout))
        assert info.width == layout


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", REFIT_SCENES)
def test_refit_blob_is_the_expected_blob(P, renderer, name, layout):
    """Both builders; after the commit (T) and after each of four updates — small jitter, large motion, every triangle shrunk to a
    quarter about its centroid (every box smaller than after `large`: a refit that only grows fails here), back to the original
    vertices — the blob has T's refs, ids and materials and the bytes expected for the current vertices, sah_cost is the exact sum within
    one float32 step, and the last blob is T again byte for byte."""
    sd = get_scene(P, name)
    for build in (0, P.native.PT_BVH_BUILD_LBVH):
        rng = np.random.default_rng(layout + build)
        renderer.SetScene(sd, layout | build)
        info, nodes, tris = blob(renderer)
        topo = (info.width, nodes, tris)
        assert info.width == layout
        check_bytes(renderer, topo, sd, (name, layout, build, "commit"))
        small = deform(sd, rng, "small")
        steps = (("small", small), ("large", deform(moved(sd, small), rng, "large")), ("shrink", shrunk(sd)), ("back", sd.verts))
        for kind, verts in steps:
            cur = moved(sd, verts)
            renderer.UpdateGeometry(verts=cur.verts)
            ctx = (name, layout, build, kind)
            info1, nodes1, tris1 = check_bytes(renderer, topo, cur, ctx)
            check_sah(info1, topo, cur, ctx)
        assert np.array_equal(nodes1, nodes) and np.array_equal(tris1, tris), (name, layout, build)


def test_shrink_through_a_device_tensor(P, renderer):
    """The `shrink` update given as a float32 torch tensor on the device (k_refit_stage) and as a numpy array: the same expected bytes."""
    import torch
    sd = get_scene(P, "tess")
    cur = moved(sd, shrunk(sd))
    for layout in (68, 73):
        for build in (0, P.native.PT_BVH_BUILD_LBVH):
            got = []
            for verts in (cur.verts, torch.from_numpy(cur.verts).cuda()):
                renderer.SetScene(sd, layout | build)
                info, nodes, tris = blob(renderer)
                topo = (info.width, nodes, tris)
                renderer.UpdateGeometry(verts=verts)
                info1, nodes1, tris1 = check_bytes(renderer, topo, cur, (layout, build, type(verts).__name__))
                check_sah(info1, topo, cur, (layout, build))
                got.append((nodes1, tris1))
            assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]), (layout, build)


def finite_in_the_reference(sd):
    """Every padded triangle box of the scene and the extent of their union (the largest extent any node has) is finite in float32."""
    box, _ = L.tri_boxes(sd.verts)
    with np.errstate(over="ignore", invalid="ignore"):
        ext = (box[:, 3:].max(0) - box[:, :3].min(0)).astype(F)
    return bool(np.isfinite(box).all() and np.isfinite(ext).all())


@pytest.mark.parametrize("k", (-30, 30, 100))
def test_scaled_scene_blob_is_the_expected_blob(P, renderer, k):
    """The tessellated box times 2^k on layouts 68 and 72, both builders: the commit's bytes and those after one large update equal
    the reference. At 2^-30 every extent is the padding; at 2^30 and 2^100 the grid exponents are 30 and 100 above the unscaled
    ones. k = 100 is included: checked here on the CPU first, in the reference alone, coordinates near 1e30 leave every box and every
    extent finite (3.4e38 is the limit). Box areas do overflow there, so sah_cost is not looked at in this test."""
    sd = S.scaled(get_scene(P, "tess"), k)
    large = moved(sd, deform(sd, np.random.default_rng(k + 100), "large"))
    assert finite_in_the_reference(sd) and finite_in_the_reference(large), k
    for layout in (68, 72):
        for build in (0, P.native.PT_BVH_BUILD_LBVH):
            renderer.SetScene(sd, layout | build)
            info, nodes, tris = blob(renderer)
            topo = (info.width, nodes, tris)
            check_bytes(renderer, topo, sd, (k, layout, build, "commit"))
            renderer.UpdateGeometry(verts=large.verts)
            check_bytes(renderer, topo, large, (k, layout, build, "large"))
