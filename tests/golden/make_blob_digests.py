"""Regenerates tests/golden/blob_digests.json: what the host builder emits (docs/SPEC.md §4.1) for a fixed set of scenes under every
node layout, as digests — SHA-256 of the node bytes and of the 48-byte triangles, n_nodes, max_depth, stack_need and the bits of
sah_cost. Detached scenes: no device. tests/test_blob_digests.py rebuilds the same scenes and compares, so that a change to the
builder, the quantiser or the record packing that moves one byte of a blob shows without a GPU. The tessellated box above 2^16
triangles goes through the threaded build and the threaded quantiser, whose output does not depend on the thread count.
Run from the repo root:  python tests/golden/make_blob_digests.py   (seconds)
"""
import hashlib
import json
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
LAYOUTS = (0, 2, 4, 68, 72, 73)
FIXTURE = os.path.join(HERE, "blob_digests.json")


def scenes(P):
    """name -> SceneData, in a fixed order."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import adversarial_scenes as A
    N = P.native
    return {
        "cornell": P.make_scene(N.PT_SCENE_CORNELL, 0, 0x5EED0001, 320, 200),
        "cornell_glass": P.make_scene(N.PT_SCENE_CORNELL_GLASS, 0, 0x5EED0001, 320, 200),
        "tess_2k": P.make_scene(N.PT_SCENE_CORNELL_TESS, 2000, 0x5EED0001, 320, 200),
        "tess_70k": P.make_scene(N.PT_SCENE_CORNELL_TESS, 70000, 0x5EED0001, 320, 200),  # 68 892 triangles: above 2^16
        "soup_5k": P.make_scene(N.PT_SCENE_TRIANGLE_SOUP, 5000, 0x5EED0001, 320, 200),
        "soup_50k": P.make_scene(N.PT_SCENE_TRIANGLE_SOUP, 50000, 0x5EED0001, 320, 200),
        "duplicates": A.duplicates(64, 64)[0],
        "stacked_layers": A.stacked_layers(64, 64),
    }


def digest(P, sd, layout):
    info, nodes, tris = P.host.build_bvh_detached(sd, layout)
    return {"width": int(info.width), "n_nodes": int(info.n_nodes), "n_tris": int(info.n_tris), "max_depth": int(info.max_depth),
            "stack_need": int(info.stack_need), "sah_cost_bits": "%08x" % struct.unpack("<I", struct.pack("<f", info.sah_cost))[0],
            "nodes_sha256": hashlib.sha256(nodes.tobytes()).hexdigest(), "tris_sha256": hashlib.sha256(tris.tobytes()).hexdigest()}


def all_digests(P):
    return {name: {str(layout): digest(P, sd, layout) for layout in LAYOUTS} for name, sd in scenes(P).items()}


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import pathtracing_amd as P
    out = all_digests(P)
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{path}: {len(out)} scenes x {len(LAYOUTS)} layouts")
