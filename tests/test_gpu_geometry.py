"""-m gpu: the device's closest hit on adversarial scenes (tests/adversarial_scenes.py), against the oracle bit for bit and
against the float64 ray caster (tests/ray_caster64.py) through primary-hit id images.

Covers what the generator scenes do not reach: traversal stacks that spill out of LDS into the overflow columns (also with
shard groups on concurrent streams), exact ties on t across leaves and Morton order, zero direction components and rays in
the plane of a wall, sphere lists up to the limit of 64, power-of-two rescaling of the whole scene (the quantisers' exponents)
and the shared-edge leak of SPEC §4's triangle test."""
import ctypes as C

import numpy as np
import pytest

import adversarial_scenes as S
import ray_caster64 as rc
from float64_support import CRACK_RAYS, PINNED_CRACKS, W, H, _size, check_classes, crack_rays, scenes
from frame_checks import _config_grid, run_both
from pipelines import flags_of
from geometry_space import SCALE_K
from trace_support import LAYOUTS

pytestmark = pytest.mark.gpu


def device_ids(P, pto, r, sd, width, w, h):
    """(device ids, oracle ids on the same blob) of the id image of `sd`."""
    img, st, ref, ost = run_both(P, pto, r, S.id_scene(sd), S.params_id(w, h), width)
    assert st.rays == ost.rays == w * h
    return S.ids_of(img), S.ids_of(ref)


def test_device_id_images_match_float64(P, pto, renderer):
    """Every adversarial scene, every layout, both builders: the device's id image equals the oracle's on the same blob, and
    its disagreements with the float64 caster are all edge or coincident-surface rays (few), or the floor camera's in-plane row."""
    LBVH = P.native.PT_BVH_BUILD_LBVH
    classes = {}
    for name, sd in scenes(P).items():
        w, h = _size(name)
        o, d = rc.camera_rays(pto, S.id_scene(sd).cam, w, h)
        cast = rc.cast(sd.verts, sd.spheres, o, d)
        for width in LAYOUTS:
            for build in (0, LBVH):
                got, want = device_ids(P, pto, renderer, sd, width | build, w, h)
                assert np.array_equal(got, want), (name, width, build, np.nonzero(got != want)[0][:10])
                c = check_classes(sd, o, d, got, name, cast)
                classes[name] = {k: len(v) for k, v in c.items() if k != "want"}
        if name == "floor":
            assert list(c["in_plane"]) == [(h // 2) * w + x for x in range(w)]
    print({k: (v["edge"], v["crack"], v["coincident"], v["in_plane"]) for k, v in classes.items()})


def test_duplicates_lowest_id_wins_on_every_kernel(P, pto, renderer):
    """Triangles repeated 9-12 times (ties on t across leaves): the lowest id wins on the device for every extend kernel, and the
    full path trace of the scene (each copy has its own material) is the oracle's."""
    N = P.native
    LBVH = N.PT_BVH_BUILD_LBVH
    sd, src = S.duplicates(W, H)
    lowest = np.array([np.nonzero(src == s)[0].min() for s in src], np.uint64)
    for flags in flags_of("probed", "simple", "packed", "pool", "split"):
        for width in (68, 2 | LBVH):
            p = S.params_id(W, H)
            p.flags = flags
            img, st, ref, ost = run_both(P, pto, renderer, S.id_scene(sd), p, width)
            ids = S.ids_of(img)
            tri = ids < len(src)
            assert tri.sum() > 0.5 * W * H
            assert np.array_equal(ids[tri], lowest[ids[tri].astype(np.int64)]), (flags, width)
            assert np.array_equal(img, ref), (flags, width)


@pytest.mark.parametrize("name", ["layers", "duplicates", "axis", "floor", "spheres64", "inside_sphere"])
def test_adversarial_scenes_full_path_trace(P, pto, renderer, name):
    """The full path trace of each adversarial scene on the configurations of _config_grid (every extend kernel counting and
    plain, every layout, both builders): frame, ray count and (counting builds) visit counters equal the oracle's."""
    sd = scenes(P, 47, 35)[name]
    for width, flags, count in _config_grid(P):
        p = P.make_params(47, 35, spp=3, max_depth=10, streams=2, flags=flags)
        img, st, ref, ost = run_both(P, pto, renderer, sd, p, width, count=count)
        ctx = (name, width, flags, count)
        assert st.rays == ost.rays and st.paths == ost.paths and np.array_equal(img, ref), ctx
        if count:
            assert (st.node_visits, st.tri_tests, st.sphere_tests) == (ost.node_visits, ost.tri_tests, ost.sphere_tests), ctx


@pytest.mark.parametrize("loops", [1, 2, 4])
def test_stacked_layers_spill_on_shard_groups(P, pto, loops):
    """The stacked-layers scene spills every ray's stack past the 12 LDS entries (test_stacked_layers_overflow_the_lds_stack).
    With the shard groups on their own streams (pt_tuning.loops) the overflow columns must not be shared: every layout and
    extend kernel renders the oracle's frame, and Render raises nothing (device error flag 1 = stack overflow)."""
    N = P.native
    LBVH = N.PT_BVH_BUILD_LBVH
    sd = S.stacked_layers(96, 64)
    r = P.Renderer(P.Window(96, 64))
    r.Init()
    try:
        r.SetTuning(loops=loops)
        for i, width in enumerate(LAYOUTS):
            for flags in flags_of("probed", "packed", "pool", "split"):
                p = P.make_params(96, 64, spp=4, max_depth=12, streams=4, flags=flags)
                img, st, ref, ost = run_both(P, pto, r, sd, p, width | (LBVH if i % 2 else 0), count=(flags == 0))
                assert r.BvhInfo().stack_need > 12
                assert st.rays == ost.rays and np.array_equal(img, ref), (loops, width, flags)
                if flags == 0:
                    assert (st.node_visits, st.tri_tests) == (ost.node_visits, ost.tri_tests), (loops, width)
    finally:
        r.Dispose()


@pytest.mark.parametrize("flags", flags_of("probed", "packed", "simple", "split", "pool"))
def test_long_sphere_lists(P, pto, renderer, flags):
    """10, 31 (the camera inside a glass ball: the t1 root), 63 and 64 spheres on every kernel: the oracle's frame, ray count and
    visit counters, with sphere_tests == n * rays. 65 spheres are refused."""
    for n, inside in ((10, False), (31, True), (63, False), (64, False)):
        sd = S.sphere_list(n, 80, 60, camera_inside=inside)
        p = P.make_params(80, 60, spp=3, max_depth=8, streams=2, flags=flags)
        img, st, ref, ost = run_both(P, pto, renderer, sd, p, 0, count=True)
        assert st.rays == ost.rays and np.array_equal(img, ref), n
        assert (st.node_visits, st.tri_tests, st.sphere_tests) == (ost.node_visits, ost.tri_tests, ost.sphere_tests), n
        assert st.sphere_tests == n * st.rays
    with pytest.raises(P.PtException):
        renderer.SetScene(S.sphere_list(65, 80, 60), 0)


def test_power_of_two_scale_is_invisible_on_the_device(P, renderer):
    """Every length times 2**k (k = -30, -8, 8, 30; ray_eps too): the device's path-traced frame is bit-identical to the unscaled
    one for every layout of both builders. Needs neither the oracle nor the caster. What it can catch is anything that does
    not scale with the scene: an absolute distance constant in the kernels (an epsilon on t, a fixed offset) or an exponent of
    the BVH4Q/8Q quantisers saturating at a clamp. A quantiser rounding error that is itself scale-invariant shifts with k in
    both frames and stays invisible here; a non-enclosing box is test_oracle_closest_hit_matches_float64's to catch.
    The ends, ±SCALE_K, are the envelope of SPEC §4's domain: at ±32 the oracle's frames change."""
    N = P.native
    LBVH = N.PT_BVH_BUILD_LBVH
    for sd in (P.make_scene(N.PT_SCENE_CORNELL, 0, 5, 48, 36), P.make_scene(N.PT_SCENE_CORNELL_GLASS, 0, 5, 48, 36),
               P.make_scene(N.PT_SCENE_CORNELL_TESS, 2000, 5, 48, 36)):
        renderer.SetScene(sd, 2)
        renderer.Params = P.make_params(48, 36, spp=2, max_depth=6)
        st0 = renderer.Render(0.0)
        ref = renderer.ReadFramebuffer()
        for k in (-SCALE_K, -8, 8, SCALE_K):
            s2 = S.scaled(sd, k)
            for width in LAYOUTS:
                for build in (0, LBVH):
                    renderer.SetScene(s2, width | build)
                    renderer.Params = P.make_params(48, 36, spp=2, max_depth=6, ray_eps=1e-4 * 2.0 ** k)
                    st = renderer.Render(0.0)
                    assert st.rays == st0.rays and np.array_equal(renderer.ReadFramebuffer(), ref), (k, width, build)


def test_device_leaks_through_the_same_shared_edges(P, pto, renderer):
    """The rays of test_shared_edge_leak_is_pinned, each traced as the only pixel of a 1x1 camera: the device misses exactly
    the rays the oracle misses (SPEC §4 is not watertight), on both builders."""
    sd, cams, o, d = crack_rays(P, pto)
    bf = pto.Scene(sd)
    want = np.array([bf.closest(o[i], d[i])[0] for i in range(CRACK_RAYS)], np.uint64)
    assert int((want == rc.MISS).sum()) == PINNED_CRACKS
    ids = S.id_scene(sd)
    for build in (0, P.native.PT_BVH_BUILD_LBVH):
        renderer.SetScene(ids, build)
        renderer.Params = S.params_id(1, 1)
        got = []
        for c in cams:
            # Renderer has no camera setter, and SetScene would rebuild the 30,000-triangle BVH for every ray. The C ABI's
            # pt_scene_set_camera changes a committed scene's camera without a re-commit, so it is called on the
            # Renderer's scene handle directly.
            cam = P.native.pt_camera.from_buffer_copy(c.cam)
            assert P.native.lib.pt_scene_set_camera(renderer._scene, C.byref(cam)) == 0
            renderer.Render(0.0)
            got.append(S.ids_of(renderer.ReadFramebuffer())[0])
        assert np.array_equal(np.array(got, np.uint64), want), build
