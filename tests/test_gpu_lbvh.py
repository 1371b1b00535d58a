"""-m gpu: the GPU BVH builder (PT_BVH_BUILD_LBVH, pathtracing_amd/csrc/lbvh.hip) against tests/lbvh_ref.py, a plain statement of what it
promises (tests/test_lbvh_ref.py holds that reference to its own checks without a device).

Any valid tree renders the same picture (docs/SPEC.md §4.1), so the structural check and the frame comparison of the other GPU tests
see almost nothing of what the builder does. Here the binary tree is read out (csrc/scene.h pt_internal_lbvh_binary) and its
triangle order, ranges, children and boxes are compared bit for bit; the committed blob's triangle order, leaves and pt_bvh_info are
recomputed from its bytes on all five layouts; the stack need it reports is driven through the overflow path; two commits give the
same bytes; and fewer than two triangles fall back to the host builder. Scenes are small: the block edges of the 256-wide launches,
the edges of the leaf size (4) and the cluster size (32), equal Morton codes, a flat axis, large offsets."""
import ctypes as C

import numpy as np
import pytest

import adversarial_scenes as S
import lbvh_ref as L
import ray_caster64 as rc
from blob_scenes import NAMES, F, blob, readout, scene
from trace_support import H, LAYOUTS, W, check_closest, commit, oracle, records

pytestmark = pytest.mark.gpu

# csrc/ptrt_internal.h PT_STACK_LDS: traversal-stack entries kept in LDS; a deeper stack spills to the overflow column. A compile-time
# constant that the library does not report: 12 is its default, which is what the Makefile builds and the suite loads
# (tools/build_variants.sh puts its -DPT_STACK_LDS=... libraries under build/variants/, which no test opens).
STACK_LDS = 12


@pytest.mark.parametrize("name", NAMES)
def test_binary_tree_equals_the_reference(P, renderer, name):
    """k_tri_boxes, k_morton, the radix sort, k_hierarchy and k_refit: the triangle order, every inner node's range and children (in
    Karras's numbering) and its box equal the reference's bit for bit."""
    sd, tree, _ = scene(P, name)
    got = readout(P, renderer, sd.verts)
    bad = L.tree_mismatches(tree, got)
    where = {k: np.nonzero(np.asarray(tree[k]).reshape(len(tree[k]), -1) != np.asarray(got[k]).reshape(len(tree[k]), -1))[0][:6].tolist() for k in bad}
    assert bad == [], (name, where)


@pytest.mark.parametrize("name", NAMES)
def test_blob_order_leaves_and_info(P, pto, renderer, name):
    """Every layout committed with the GPU builder: every leaf of the blob holds the triangle ids of one leaf of the reference's partition,
    in the reference's order, and every reference leaf is there — so the device packer (68) and the host packer (2, 4, 72, 73) cut the
    same leaves out of the same tree. Layout 68 keeps the triangles in Morton order, so there the ids in array order are the reference's
    order and the leaf ranges are the reference's ranges; the host packer emits the leaves in the order of its breadth-first walk
    (docs/SPEC.md §4.1; octant slots permute it again), so there the leaves are compared by their ids. n_nodes, max_depth
    and stack_need of pt_bvh_info equal a walk of the bytes, node_bytes = n_nodes * stride, sah_cost is the SPEC §4.3 sum over exact
    boxes within 1e-5 (the bound tests/test_gpu_update.py holds this quantity to); the blob passes the oracle's structural check and
    a 48 x 36 frame equals the oracle traversing the same bytes.

    Each commit prints the reported sah_cost, the recomputed one and their relative difference (pytest -s): the host packer's figure
    (layouts 2, 4, 72, 73) is the same float64 sum rounded to float32, at most 6e-8 away; the device packer's (68) takes every term as
    area * (1 / root area) in float32 and sums in float32, a few 1e-7 by the error bounds of those operations on these node counts."""
    N = P.native
    sd, tree, leaves = scene(P, name)
    params = P.make_params(W, H, spp=1, max_depth=3)
    for layout in LAYOUTS:
        osc = commit(P, pto, renderer, sd, layout | N.PT_BVH_BUILD_LBVH)  # validate_bvh() == 0
        info, nodes, tris = blob(renderer)
        ctx = (name, layout)
        assert info.width == layout and info.n_tris == len(sd.verts), ctx
        if layout == 68:  # packed on the device: triangles in Morton order, so a leaf's range is the reference's range
            assert np.array_equal(L.blob_order(tris), tree["order"]), ctx
            assert L.leaves_of(layout, nodes) == leaves, ctx
        else:  # packed by the host from the read-back tree: the same leaves, emitted in the order of its breadth-first walk
            assert sorted(c for _, c in L.leaves_of(layout, nodes)) == sorted(c for _, c in leaves), ctx
        assert L.leaf_ids(layout, nodes, tris) == L.partition_ids(tree, leaves), ctx
        assert L.info_mismatches(info, layout, nodes, tris, sd.verts) == [], ctx
        renderer.Params = params
        st = renderer.Render(0.0)
        ref, ost = pto.render(osc, params)
        assert np.array_equal(renderer.ReadFramebuffer(), ref) and (st.rays, st.paths) == (ost.rays, ost.paths), ctx


def test_stack_need_is_reachable(P, pto, renderer):
    """The layers scene: the stack need recomputed from the bytes equals the reported one, it is deeper than the LDS part of the traversal
    stack on the host-packed layouts (the host packer, run on the reference tree, gives 13, 24, 35 and 35 for 2, 4, 72 and 73), and it is what
    sizes the overflow column. A 64 x 48 frame of 2 spp and a batch of ray queries go through the overflow path without the device's
    error flag (Render and TraceRays raise on it) and equal the oracle."""
    N = P.native
    sd = S.stacked_layers(64, 48)
    params = P.make_params(64, 48, spp=2, max_depth=8)
    o, d = rc.camera_rays(pto, sd.cam, 64, 48)
    for layout in LAYOUTS:
        osc = commit(P, pto, renderer, sd, layout | N.PT_BVH_BUILD_LBVH)
        info, nodes, _ = blob(renderer)
        need = L.walk_info(layout, nodes)[2]
        assert info.stack_need == need and need > STACK_LDS, (layout, info.stack_need, need)
        renderer.Params = params
        st = renderer.Render(0.0)
        ref, ost = pto.render(osc, params)
        assert np.array_equal(renderer.ReadFramebuffer(), ref) and st.rays == ost.rays, layout
        ids, ts, _ = oracle(pto, osc, o, d)
        hits, qst = renderer.TraceRays(records(o, d))
        check_closest(hits, ids, ts, layout)
        assert qst.rays == len(o)


@pytest.mark.parametrize("name", ["soup3000", "tess2000", "same300"])
def test_commit_twice_same_bytes(P, renderer, name):
    """k_mark appends clusters through an atomic and the host sorts them: two commits of one scene give the same node bytes, triangle
    bytes and info (build_ms apart)."""
    sd = scene(P, name)[0]
    for layout in (68, 4):
        out = []
        for _ in range(2):
            renderer.SetScene(sd, layout | P.native.PT_BVH_BUILD_LBVH)
            out.append(blob(renderer))
        (ia, na, ta), (ib, nb, tb) = out
        assert np.array_equal(na, nb) and np.array_equal(ta, tb), (name, layout)
        for k in ("width", "n_nodes", "n_tris", "max_depth", "node_bytes", "tri_bytes", "stack_need"):
            assert getattr(ia, k) == getattr(ib, k), (name, layout, k)
        assert np.float32(ia.sah_cost).view(np.uint32) == np.float32(ib.sah_cost).view(np.uint32), (name, layout)


@pytest.mark.parametrize("n", [0, 1])
def test_fewer_than_two_triangles_fall_back(P, renderer, n):
    """With the builder flag, 0 and 1 triangles commit and give exactly the host builder's blob, on every layout; the read-out refuses
    them, and NULL pointers, with PT_ERR_INVALID_ARGUMENT."""
    N = P.native
    sd = S._clone(P.make_scene(N.PT_SCENE_CORNELL, 0, 1, W, H))
    sd.verts, sd.tri_mat = sd.verts[3:3 + n].copy(), sd.tri_mat[3:3 + n].copy()
    for layout in LAYOUTS:
        renderer.SetScene(sd, layout | N.PT_BVH_BUILD_LBVH)
        info, nodes, tris = blob(renderer)
        hinfo, hnodes, htris = P.host.build_bvh_detached(sd, layout)
        assert np.array_equal(nodes, hnodes) and np.array_equal(tris, htris), layout
        assert (info.width, info.n_nodes, info.n_tris, info.max_depth, info.stack_need, info.sah_cost, info.node_bytes, info.tri_bytes) == \
            (hinfo.width, hinfo.n_nodes, hinfo.n_tris, hinfo.max_depth, hinfo.stack_need, hinfo.sah_cost, hinfo.node_bytes, hinfo.tri_bytes), layout
        assert L.info_mismatches(info, layout, nodes, tris, sd.verts) == [] and info.n_nodes == n
    buf = np.zeros(64, np.uint32)
    p = buf.ctypes.data_as(C.c_void_p)
    v = np.array(scene(P, "random5")[0].verts, F).reshape(5, 9)  # a copy: a coordinate is overwritten below
    call = N.lib.pt_internal_lbvh_binary
    assert call(renderer._ctx, v.ctypes.data_as(C.c_void_p), n, p, p, p, p, p, p) == N.PT_ERR_INVALID_ARGUMENT
    assert call(renderer._ctx, None, 5, p, p, p, p, p, p) == N.PT_ERR_INVALID_ARGUMENT
    assert call(renderer._ctx, v.ctypes.data_as(C.c_void_p), 5, p, p, p, p, p, None) == N.PT_ERR_INVALID_ARGUMENT
    assert call(None, v.ctypes.data_as(C.c_void_p), 5, p, p, p, p, p, p) == N.PT_ERR_INVALID_ARGUMENT
    # the limits pt_scene_set_triangles puts before the builder: fewer than 2^28 triangles (refused before anything is read), finite coordinates
    assert call(renderer._ctx, v.ctypes.data_as(C.c_void_p), 1 << 28, p, p, p, p, p, p) == N.PT_ERR_INVALID_ARGUMENT
    v[4, 8] = np.nan
    assert call(renderer._ctx, v.ctypes.data_as(C.c_void_p), 5, p, p, p, p, p, p) == N.PT_ERR_INVALID_ARGUMENT
    assert not buf.any()  # and nothing was written
