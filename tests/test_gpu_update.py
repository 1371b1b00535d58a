"""-m gpu: pt_scene_update_triangles / pt_scene_update_spheres (docs/SPEC.md §4.3) against the oracle, on every layout and both builders.

A refit keeps the committed tree's topology and recomputes the triangle records and every box from the new vertices, so the blob it
leaves must pass the oracle's structural check against the new vertices, render the oracle's frame bit for bit, answer ray queries as
the oracle does, and give the frame of a fresh commit of the moved geometry. Also: a no-op update changes no byte, device and host
input agree, spheres move, topology and sah_cost behave, long animations and a re-commit work, a refused device update changes
nothing, progressive rendering is undisturbed, and a 1M-triangle tree refits."""
import ctypes as C

import numpy as np
import pytest

from lbvh_ref import numpy_sah
from blob_scenes import SCENES, blob, deform, moved
from frame_checks import check_against_oracle
from trace_support import H, LAYOUTS, W, scenes

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", SCENES)
def test_refit_is_exact(P, pto, renderer, name):
    """Small jitter, then large motion, on every layout and builder: the refitted blob validates against the new vertices and the
    device equals the oracle on it (frames, rays, paths, closest hits, visit counters)."""
    N = P.native
    sd = scenes(P)[name]
    for width in LAYOUTS:
        for build in (0, N.PT_BVH_BUILD_LBVH):
            rng = np.random.default_rng(width + build)
            renderer.SetScene(sd, width | build)
            cur = sd
            for kind in ("small", "large"):
                cur = moved(sd, deform(cur, rng, kind))
                st = renderer.UpdateGeometry(verts=cur.verts)
                assert st.rays == 0 and st.node_visits == 0 and (st.gpu_ms > 0) == (len(cur.verts) > 0)
                check_against_oracle(P, pto, renderer, cur, (name, width, build, kind))


@pytest.mark.parametrize("name", ["glass", "tess", "soup"])
def test_same_picture_as_a_rebuild(P, pto, renderer, name):
    """The frame after an update equals the frame from a fresh SetScene of the deformed geometry, bit for bit."""
    N = P.native
    sd = scenes(P)[name]
    params = P.make_params(W, H, spp=4, max_depth=8, streams=4)
    for width in LAYOUTS:
        for build in (0, N.PT_BVH_BUILD_LBVH):
            v2 = deform(sd, np.random.default_rng(7), "large")
            renderer.SetScene(sd, width | build)
            renderer.UpdateGeometry(verts=v2)
            renderer.Params = params
            renderer.Render(0.0)
            refit = renderer.ReadFramebuffer()
            renderer.SetScene(moved(sd, v2), width | build)
            renderer.Render(0.0)
            assert np.array_equal(refit, renderer.ReadFramebuffer()), (name, width, build)


@pytest.mark.parametrize("name", ["glass", "tess", "soup", "duplicates"])
def test_noop_update_changes_nothing(P, pto, renderer, name):
    """Every builder puts exact unions of the padded triangle boxes in its blob, and the refit computes the same unions with the same
    quantiser: updating with the unchanged vertices leaves every byte as the commit made it, and sah_cost within 1e-5."""
    N = P.native
    sd = scenes(P)[name]
    for width in LAYOUTS:
        for build in (0, N.PT_BVH_BUILD_LBVH):
            renderer.SetScene(sd, width | build)
            info0, nodes0, tris0 = blob(renderer)
            for _ in range(2):
                renderer.UpdateGeometry(verts=sd.verts)
                info1, nodes1, tris1 = blob(renderer)
                assert np.array_equal(nodes0, nodes1) and np.array_equal(tris0, tris1), (name, width, build)
                assert abs(info1.sah_cost - info0.sah_cost) <= 1e-5 * info0.sah_cost, (name, width, build, info0.sah_cost, info1.sah_cost)
                assert info1.build_ms == info0.build_ms


def test_device_input_equals_host_input(P, pto, renderer):
    """A float32 torch tensor on the device and a numpy array give identical blob bytes and sah_cost."""
    import torch
    N = P.native
    sd = scenes(P)["tess"]
    v2 = deform(sd, np.random.default_rng(3), "large")
    for width in (2, 68, 73):
        for build in (0, N.PT_BVH_BUILD_LBVH):
            out = []
            for verts in (v2, torch.from_numpy(v2).cuda(), torch.from_numpy(v2.reshape(-1, 3, 3)).cuda()):
                renderer.SetScene(sd, width | build)
                st = renderer.UpdateGeometry(verts=verts)
                assert st.gpu_ms > 0
                out.append(blob(renderer))
            for info, nodes, tris in out[1:]:
                assert np.array_equal(nodes, out[0][1]) and np.array_equal(tris, out[0][2]), (width, build)
                assert info.sah_cost == out[0][0].sah_cost


def test_spheres_move(P, pto, renderer):
    """Moved and resized spheres (triangles unchanged, then both at once) give the oracle's frame."""
    sd = scenes(P)["spheres64"]
    rng = np.random.default_rng(5)
    for width in (2, 68):
        renderer.SetScene(sd, width)
        sph = np.asarray(sd.spheres, np.float32).copy()
        sph[:, :3] += rng.normal(scale=0.05, size=(len(sph), 3)).astype(np.float32)
        sph[:, 3] *= rng.uniform(0.5, 1.5, size=len(sph)).astype(np.float32)
        st = renderer.UpdateGeometry(spheres=sph)
        assert st.gpu_ms == 0
        check_against_oracle(P, pto, renderer, moved(sd, spheres=sph), ("spheres", width))
        v2 = deform(sd, rng, "small")
        sph2 = sph.copy()
        sph2[:, 1] += np.float32(0.1)
        renderer.UpdateGeometry(verts=v2, spheres=sph2)
        check_against_oracle(P, pto, renderer, moved(sd, v2, sph2), ("both", width))


def test_topology_stable_and_sah(P, pto, renderer):
    """n_nodes, max_depth, stack_need and the layout stay through updates; sah_cost rises with large motion, and on the f32 layouts
    equals a numpy recomputation from the read-back boxes within 1e-5. (numpy_sah takes the blob's own boxes; the refit's sah_cost against
    exact boxes recomputed from the vertices, on the quantised layouts 68, 72 and 73 too and within one float32 step, is
    tests/test_gpu_blob_ref.py test_refit_blob_is_the_expected_blob's.)"""
    N = P.native
    for name in ("tess", "soup", "layers"):
        sd = scenes(P)[name]
        for width in LAYOUTS:
            for build in (0, N.PT_BVH_BUILD_LBVH):
                renderer.SetScene(sd, width | build)
                info0, nodes0, _ = blob(renderer)
                if width in (2, 4):
                    assert abs(numpy_sah(nodes0, width) - info0.sah_cost) <= 1e-5 * info0.sah_cost
                renderer.UpdateGeometry(verts=deform(sd, np.random.default_rng(1), "large"))
                info1, nodes1, _ = blob(renderer)
                ctx = (name, width, build)
                assert (info1.width, info1.n_nodes, info1.max_depth, info1.stack_need, info1.node_bytes, info1.tri_bytes) == \
                    (info0.width, info0.n_nodes, info0.max_depth, info0.stack_need, info0.node_bytes, info0.tri_bytes), ctx
                assert info1.sah_cost > info0.sah_cost, ctx
                if width in (2, 4):
                    assert abs(numpy_sah(nodes1, width) - info1.sah_cost) <= 1e-5 * info1.sah_cost, ctx


def test_long_animation_and_recommit(P, pto, renderer):
    """Ten consecutive updates (a wave through the mesh) all validate and match the oracle; a pt_scene_commit after them builds from
    the updated geometry."""
    N = P.native
    sd = scenes(P)["tess"]
    v = np.asarray(sd.verts, np.float32).reshape(-1, 3, 3)
    ext = float(np.ptp(v.reshape(-1, 3), axis=0).max())
    for width, build in ((68, N.PT_BVH_BUILD_LBVH), (73, 0), (4, 0)):
        renderer.SetScene(sd, width | build)
        cur = sd
        for k in range(10):
            w = v.copy()
            w[..., 1] += (0.05 * ext * np.sin(w[..., 0] * 7.0 + k * 0.6)).astype(np.float32)
            cur = moved(sd, w)
            renderer.UpdateGeometry(verts=cur.verts)
            if k % 3 == 0 or k == 9:
                check_against_oracle(P, pto, renderer, cur, (width, build, k))
            else:
                info, nodes, tris = blob(renderer)
                assert pto.Scene(cur, (info.width, nodes, tris)).validate_bvh()[0] == 0
        assert N.lib.pt_scene_commit(renderer._scene, width | build) == N.PT_OK
        check_against_oracle(P, pto, renderer, cur, (width, build, "recommit"))


def test_reads_between_updates_then_recommit_elsewhere(P, pto, renderer):
    """The blob read before and between updates (the second of two reads in a row comes from the host copy the first one fetched), a
    host update and a device update, then pt_scene_commit with another layout and the other builder: the commit builds from the
    twice-moved vertices. A host-built target equals a fresh SetScene of those vertices byte for byte; an LBVH target validates and
    renders the oracle's frame."""
    import torch
    N = P.native
    L = N.PT_BVH_BUILD_LBVH
    sd = scenes(P)["tess"]
    rng = np.random.default_rng(11)
    v1 = deform(sd, rng, "large")
    v2 = deform(moved(sd, v1), rng, "large")
    for start, target in ((68 | L, 4), (68, 2), (2, 68 | L), (73, 68)):
        ctx = (start, target)
        renderer.SetScene(sd, start)
        blob(renderer)
        renderer.UpdateGeometry(verts=v1)
        (_, nodes_a, tris_a), (_, nodes_b, tris_b) = blob(renderer), blob(renderer)
        assert np.array_equal(nodes_a, nodes_b) and np.array_equal(tris_a, tris_b), ctx
        renderer.UpdateGeometry(verts=torch.from_numpy(v2).cuda())
        assert N.lib.pt_scene_commit(renderer._scene, target) == N.PT_OK, ctx
        cur = moved(sd, v2)
        check_against_oracle(P, pto, renderer, cur, ctx)
        info, nodes, tris = blob(renderer)
        assert info.width == target & ~L, ctx
        if target & L:
            continue  # (validate_bvh() == 0 and the oracle's frame: check_against_oracle)
        renderer.SetScene(cur, target)
        info1, nodes1, tris1 = blob(renderer)
        assert np.array_equal(nodes, nodes1) and np.array_equal(tris, tris1), ctx
        assert (info.n_nodes, info.max_depth, info.stack_need, info.sah_cost) == (info1.n_nodes, info1.max_depth, info1.stack_need, info1.sah_cost), ctx


def test_refused_device_update_changes_nothing(P, pto, renderer):
    """A device array with one NaN is PT_ERR_INVALID_ARGUMENT, and the blob and the next frame equal those before the call; so are a
    device pointer that is not 4-byte aligned, host memory passed as device memory, and a wrong count."""
    import torch
    N = P.native
    sd = scenes(P)["glass"]
    for width in (2, 68):
        renderer.SetScene(sd, width)
        renderer.UpdateGeometry(verts=deform(sd, np.random.default_rng(2), "small"))
        info0, nodes0, tris0 = blob(renderer)
        renderer.Params = P.make_params(W, H, spp=4, max_depth=8, streams=4)
        renderer.Render(0.0)
        before = renderer.ReadFramebuffer()
        bad = torch.from_numpy(deform(sd, np.random.default_rng(4), "large")).cuda()
        bad[len(bad) // 2, 4] = float("nan")
        host = np.asarray(sd.verts, np.float32).copy()
        torch.cuda.synchronize()
        st = N.pt_stats()
        call = lambda p, n: N.lib.pt_scene_update_triangles(renderer._scene, C.c_void_p(p), n, 0, C.byref(st))
        assert call(bad.data_ptr(), len(bad)) == N.PT_ERR_INVALID_ARGUMENT
        assert b"non-finite" in N.lib.pt_last_error(renderer._ctx)
        assert call(bad.data_ptr() + 2, len(bad)) == N.PT_ERR_INVALID_ARGUMENT
        assert call(host.ctypes.data, len(bad)) == N.PT_ERR_INVALID_ARGUMENT
        assert b"not device memory" in N.lib.pt_last_error(renderer._ctx)
        assert call(bad.data_ptr(), len(bad) - 1) == N.PT_ERR_INVALID_ARGUMENT
        with pytest.raises(P.PtException):
            renderer.UpdateGeometry(verts=bad)
        info1, nodes1, tris1 = blob(renderer)
        assert np.array_equal(nodes0, nodes1) and np.array_equal(tris0, tris1) and info1.sah_cost == info0.sah_cost
        renderer.Render(0.0)
        assert np.array_equal(renderer.ReadFramebuffer(), before), width


def test_progressive_frames_then_update(P, pto, renderer):
    """Progressive frames (PT_FLAG_ACCUMULATE), an update, then a non-accumulate frame with spp >= streams: the oracle's frame of the
    new geometry. The update keeps the scene's extend-kernel choice and the context's frame-start template; neither may show."""
    N = P.native
    sd = scenes(P)["glass"]
    renderer.SetScene(sd, 0)
    for offset, flags in ((0, 0), (4, N.PT_FLAG_ACCUMULATE), (8, N.PT_FLAG_ACCUMULATE)):
        renderer.Params = P.make_params(W, H, spp=4, max_depth=8, streams=4, sample_offset=offset, flags=flags)
        renderer.Render(0.0)
    v2 = deform(sd, np.random.default_rng(9), "large")
    renderer.UpdateGeometry(verts=v2)
    for spp in (4, 8):
        check_against_oracle(P, pto, renderer, moved(sd, v2), spp, P.make_params(W, H, spp=spp, max_depth=8, streams=4))


def test_million_triangle_lbvh_refits(P, pto, renderer):
    """The 1M-triangle Cornell box committed with the GPU builder (BVH4Q packed on the device), deformed on the device: the blob still
    validates, the topology stays, and a small frame matches the oracle."""
    import torch
    N = P.native
    sd = P.make_scene(N.PT_SCENE_CORNELL_TESS, 1_000_000, 3, W, H)
    renderer.SetScene(sd, N.PT_BVH_BUILD_LBVH)
    info0 = renderer.BvhInfo()
    assert info0.width == 68 and info0.n_tris >= 900_000
    v = torch.from_numpy(np.asarray(sd.verts, np.float32)).cuda().reshape(-1, 3, 3)
    v = v + 0.02 * torch.sin(v[..., 0:1] * 5.0)
    st = renderer.UpdateGeometry(verts=v)
    assert st.gpu_ms > 0
    cur = moved(sd, v.cpu().numpy())
    info1 = renderer.BvhInfo()
    assert (info1.n_nodes, info1.max_depth, info1.stack_need) == (info0.n_nodes, info0.max_depth, info0.stack_need)
    check_against_oracle(P, pto, renderer, cur, "1M", P.make_params(W, H, spp=1, max_depth=4))
