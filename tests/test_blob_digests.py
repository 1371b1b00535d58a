"""The host builder's blobs, byte for byte: every scene of tests/golden/make_blob_digests.py under every node layout must still give
the digests recorded in tests/golden/blob_digests.json (node bytes, triangle bytes, n_nodes, max_depth, stack_need, sah_cost bits).
No device: detached scenes. The rules these bytes follow are stated once, in pathtracing_amd/csrc/blob_rules.h, for the host builder,
the GPU builder and the refit; the GPU suite holds the GPU builder to a plain reference of its tree, leaves and info
(tests/test_gpu_lbvh.py) and the refit to the host's and the commit's bytes (tests/test_gpu_update.py)."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_blob_digests", os.path.join(GOLDEN, "make_blob_digests.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

SCENES = ("cornell", "cornell_glass", "tess_2k", "tess_70k", "soup_5k", "soup_50k", "duplicates", "stacked_layers")


@pytest.fixture(scope="module")
def built_scenes(P):
    sc = M.scenes(P)
    assert tuple(sc) == SCENES
    return sc


@pytest.fixture(scope="module")
def golden():
    with open(M.FIXTURE) as f:
        g = json.load(f)
    assert set(g) == set(SCENES) and all(set(v) == {str(x) for x in M.LAYOUTS} for v in g.values())
    return g


@pytest.mark.parametrize("layout", M.LAYOUTS)
@pytest.mark.parametrize("scene", SCENES)
def test_host_blob_matches_recorded_digest(P, built_scenes, golden, scene, layout):
    assert M.digest(P, built_scenes[scene], layout) == golden[scene][str(layout)]
