"""Regenerates tests/golden/lbvh_blob_digests.json: what a commit with the GPU builder (layout | PT_BVH_BUILD_LBVH) leaves in the scene,
as the digests of tests/golden/make_blob_digests.py — width, n_nodes, n_tris, max_depth, stack_need, the bits of sah_cost, SHA-256 of
the node bytes and of the 48-byte triangles — taken from BvhInfo() / BvhRead(). Needs a device. tests/test_gpu_lbvh_digests.py commits
the same scenes and compares exactly, so that a change to the cut, the top storey, the collapse (which 4-wide nodes k_expand or
emit_blob form) or the figures shows, which the reference checks of test_gpu_lbvh.py and test_gpu_blob_ref.py leave free.
Scenes: the 27 of tests/test_gpu_lbvh.py, and a 300 k-triangle soup whose cluster count (recorded here, from tests/lbvh_ref.py) lies
above the 8192 boxes from which build_sah_over_boxes builds on threads. "commit" is the commit whose csrc/ made the file.
Run from the repo root:  python tests/golden/make_lbvh_blob_digests.py <commit id> [path]   (half a minute, most of it the reference)
"""
import hashlib
import json
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "lbvh_blob_digests.json")
BIG = "soup300k"
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)


def scenes(P):
    """name -> SceneData, in a fixed order."""
    import test_gpu_lbvh as T
    out = {name: T.scene(P, name)[0] for name in T.NAMES}
    out[BIG] = P.make_scene(P.native.PT_SCENE_TRIANGLE_SOUP, 300000, 3, T.W, T.H)
    return out


def layouts():
    import test_gpu_lbvh as T
    return tuple(T.LAYOUTS)


def digest(P, r, sd, layout):
    r.SetScene(sd, layout | P.native.PT_BVH_BUILD_LBVH)
    info = r.BvhInfo()
    nodes, tris = r.BvhRead()
    return {"width": int(info.width), "n_nodes": int(info.n_nodes), "n_tris": int(info.n_tris), "max_depth": int(info.max_depth),
            "stack_need": int(info.stack_need), "sah_cost_bits": "%08x" % struct.unpack("<I", struct.pack("<f", info.sah_cost))[0],
            "nodes_sha256": hashlib.sha256(nodes.tobytes()).hexdigest(), "tris_sha256": hashlib.sha256(tris.tobytes()).hexdigest()}


if __name__ == "__main__":
    import lbvh_ref as L
    import pathtracing_amd as P
    sc = scenes(P)
    r = P.Renderer(P.Window(64, 64))
    r.Init()
    try:
        blobs = {name: {str(layout): digest(P, r, sd, layout) for layout in layouts()} for name, sd in sc.items()}
    finally:
        r.Dispose()
    out = {"commit": sys.argv[1], "clusters": {BIG: len(L.leaf_partition(L.build(sc[BIG].verts))[1])}, "blobs": blobs}
    path = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{path}: {len(blobs)} scenes x {len(layouts())} layouts; {BIG}: {out['clusters'][BIG]} clusters")
