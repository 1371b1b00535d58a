"""-m gpu: the GPU builder's blobs, byte for byte. Every scene of tests/golden/make_lbvh_blob_digests.py, committed with
layout | PT_BVH_BUILD_LBVH under the five layouts, must still give the digests recorded in tests/golden/lbvh_blob_digests.json: node
bytes, triangle bytes, n_nodes, max_depth, stack_need and the bits of sah_cost, with no tolerance and nothing left out.
tests/test_gpu_lbvh.py holds the leaves and the figures to a reference and tests/test_gpu_blob_ref.py every byte that a topology
determines; which 4-wide nodes the device packer (68) or the host packer (2, 4, 72, 73) forms, and what the top storey over the
clusters looks like, is fixed only here. The 300 k-triangle soup has more clusters than the 8192 boxes from which the top storey is
built on threads; the fixture records their number, this test only commits and hashes."""
import importlib.util
import json
import os

import pytest

from blob_scenes import NAMES
from trace_support import LAYOUTS

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_lbvh_blob_digests", os.path.join(GOLDEN, "make_lbvh_blob_digests.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

SCENES = tuple(NAMES) + (M.BIG,)


@pytest.fixture(scope="module")
def built_scenes(P):
    sc = M.scenes(P)
    assert tuple(sc) == SCENES
    return sc


@pytest.fixture(scope="module")
def golden():
    with open(M.FIXTURE) as f:
        g = json.load(f)
    assert set(g["blobs"]) == set(SCENES) and all(set(v) == {str(x) for x in LAYOUTS} for v in g["blobs"].values())
    assert g["clusters"][M.BIG] > 8192  # bvh_build.cpp build_sah_over_boxes: the threaded top storey
    return g["blobs"]


@pytest.mark.parametrize("scene", SCENES)
def test_lbvh_blob_matches_recorded_digest(P, renderer, built_scenes, golden, scene):
    for layout in LAYOUTS:
        assert M.digest(P, renderer, built_scenes[scene], layout) == golden[scene][str(layout)], (scene, layout)
