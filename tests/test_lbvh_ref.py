"""tests/lbvh_ref.py earns its trust without a device, before tests/test_gpu_lbvh.py lets it judge the GPU builder.

The blob checkers (walk_info, exact_sah, leaves_of) are run on the host builder's detached blobs, an independent producer whose info is
pinned by tests/golden/blob_digests.json; the radix tree is held to its defining invariants on random and adversarial code arrays; the
Morton quantiser to hand-derived values at its edges; the leaf rule to two-triangle cases worked out by hand; and every comparison the
GPU tests make is shown to reject an input with one thing changed."""
import importlib.util
import math
import os
import types

import numpy as np
import pytest

import lbvh_ref as L
from trace_support import LAYOUTS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_blob_digests", os.path.join(GOLDEN, "make_blob_digests.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

SCENES = ("cornell", "tess_2k", "soup_5k", "duplicates", "stacked_layers")
F = np.float32


@pytest.fixture(scope="module")
def scenes(P):
    sc = M.scenes(P)
    return {k: sc[k] for k in SCENES}


@pytest.fixture(scope="module")
def blobs(P, scenes):
    cache = {}

    def get(scene, layout):
        if (scene, layout) not in cache:
            info, nodes, tris = P.host.build_bvh_detached(scenes[scene], layout)
            cache[scene, layout] = (info, nodes.copy(), tris.copy())
        return cache[scene, layout]
    return get


# ---------------------------------------------------------------------------------------------- checkers against the host builder

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("scene", SCENES)
def test_checkers_agree_with_the_host_builder(scenes, blobs, scene, layout):
    """(n_nodes, max_depth, stack_need) of the host builder's info equal walk_info of its bytes, sah_cost is exact_sah within 1e-5
    (the bound of tests/test_gpu_update.py), and the leaves tile the triangle array with the ids a permutation."""
    info, nodes, tris = blobs(scene, layout)
    sd = scenes[scene]
    assert info.width == layout and info.node_bytes == info.n_nodes * L.STRIDE[layout]
    assert L.walk_info(layout, nodes) == (info.n_nodes, info.max_depth, info.stack_need)
    sah = L.exact_sah(layout, nodes, tris, sd.verts)
    assert abs(sah - info.sah_cost) <= 1e-5 * sah, (sah, info.sah_cost)
    assert L.info_mismatches(info, layout, nodes, tris, sd.verts) == []
    pos = 0
    for first, count in L.leaves_of(layout, nodes):
        assert first == pos and 1 <= count <= 4
        pos += count
    assert pos == len(sd.tri_mat)
    assert np.array_equal(np.sort(L.blob_order(tris)), np.arange(len(sd.tri_mat)))


def test_exact_sah_equals_the_f32_slots(scenes, blobs):
    """On layouts 2 and 4 the blob stores the exact boxes, so exact_sah must equal the sum taken from the stored slots."""
    for scene in SCENES:
        for layout in (2, 4):
            _, nodes, tris = blobs(scene, layout)
            a, b = L.exact_sah(layout, nodes, tris, scenes[scene].verts), L.numpy_sah(nodes, layout)
            assert abs(a - b) <= 1e-12 * b, (scene, layout, a, b)  # the same float64 terms, summed in another order


def test_empty_blob():
    assert L.walk_info(68, np.zeros(0, np.uint8)) == (0, 0, 0) and L.leaves_of(4, np.zeros(0, np.uint8)) == []
    assert L.exact_sah(2, np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros((0, 9), F)) == 0.0


# ---------------------------------------------------------------------------------------------- triangle boxes and Morton codes

def test_tri_boxes_by_hand():
    v = F([[0, 0, 0, 1, 2, -3, 0.5, -100, 4], [-0.0, 5, 5, 0.0, 5, 5, 0.0, 5, 5]])
    box, cent = L.tri_boxes(v)
    e = F(1e-6)
    want = F([[F(0) - e, F(-100) - e * F(100), F(-3) - e * F(3), F(1) + e, F(2) + e * F(2), F(4) + e * F(4)],
              [F(0) - e, F(5) - e * F(5), F(5) - e * F(5), F(0) + e, F(5) + e * F(5), F(5) + e * F(5)]])
    assert np.array_equal(box, want) and box.dtype == F
    assert np.array_equal(cent, F([[0.5, -49, 0.5], [0, 5, 5]]))
    assert (box[:, :3] < v.reshape(-1, 3, 3).min(1)).all() and (box[:, 3:] > v.reshape(-1, 3, 3).max(1)).all()


def test_morton_edges_by_hand():
    """x runs 0 .. 1 (the upper bound must give 1023, not 1024), y is flat (0), z has two values 1e-40 apart (inv = inf: 0 and 1023,
    no NaN). Bit 29 is x's top bit, bit 28 y's, bit 27 z's."""
    cent = F([[0, 7, 0], [1, 7, 1e-40], [0.5, 7, 0], [0.25, 7, 1e-40]])
    q = L.quantise_centroids(cent)
    assert q.tolist() == [[0, 0, 0], [1023, 0, 1023], [512, 0, 0], [256, 0, 1023]]
    codes = L.morton_codes(cent)

    def interleave(x, y, z):
        return sum(((x >> b & 1) << 3 * b + 2) | ((y >> b & 1) << 3 * b + 1) | ((z >> b & 1) << 3 * b) for b in range(10))
    assert codes.tolist() == [interleave(*row) for row in q.tolist()]
    assert codes[2] == 1 << 29 and codes[3] == (1 << 26) | 0x09249249 and codes.max() < 1 << 30
    assert L.morton_codes(F([[1, 0, 0], [0, 0, 0]])).tolist() == [0x24924924, 0]  # x alone: every third bit from bit 2
    assert L.morton_codes(F([[0, 0, 1], [0, 0, 0]])).tolist() == [0x09249249, 0]


def test_morton_signed_zero_and_negative_bounds():
    """Bounds that span -0.0 / +0.0 are flat; negative coordinates quantise from their own minimum."""
    assert L.quantise_centroids(F([[-0.0, 0, 0], [0.0, 0, 0]])).tolist() == [[0, 0, 0], [0, 0, 0]]
    q = L.quantise_centroids(F([[-3, -1e4, -0.0], [-1, -1e4 + 1, 0.0], [-2, -1e4 + 0.5, 0.0]]))
    assert q.tolist() == [[0, 0, 0], [1023, 1023, 0], [512, 512, 0]]
    same = L.quantise_centroids(F([[2.5, -2.5, 1e30]] * 5))
    assert (same == 0).all()


def test_order_is_stable():
    codes = np.array([5, 1, 5, 1, 0, 5], np.uint32)
    assert L.sort_order(codes).tolist() == [4, 1, 3, 0, 2, 5]


# ---------------------------------------------------------------------------------------------- the radix tree

def _code_arrays():
    rng = np.random.default_rng(2024)
    out = {}
    for n in (2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 100, 255, 256, 257, 600):
        out[f"random{n}"] = np.sort(rng.integers(0, 1 << 30, n, dtype=np.uint32))
        out[f"equal{n}"] = np.full(n, 0x2AAAAAAA, np.uint32)
        out[f"two{n}"] = np.sort(rng.choice(np.array([3, 1 << 29], np.uint32), n))
        out[f"runs{n}"] = np.sort(rng.integers(0, max(2, n // 6), n, dtype=np.uint32) * np.uint32(0x01000193 & 0x3FFFFFF))
        out[f"dense{n}"] = np.sort(rng.integers(0, 16, n, dtype=np.uint32))
    return out


CODES = _code_arrays()


def _prefix(a, b):
    return 64 - (a ^ b).bit_length()


@pytest.mark.parametrize("name", sorted(CODES))
def test_radix_tree_invariants(name):
    codes = CODES[name]
    n = len(codes)
    t = L.radix_tree(codes)
    keys = [(int(c) << 32) | i for i, c in enumerate(codes)]
    assert all(len(t[k]) == n - 1 for k in ("left", "right", "first", "last"))
    assert (t["first"][0], t["last"][0]) == (0, n - 1)
    leaf_seen, node_seen = np.zeros(n, int), np.zeros(n - 1, int)
    node_seen[0] = 1
    for i in range(n - 1):
        f, l, g = int(t["first"][i]), int(t["last"][i]), int(t["split"][i])
        assert f <= g < l
        # the range is split where the common prefix of its keys ends: both halves share more of the key than the range does, and the
        # keys just outside the range share less
        whole = _prefix(keys[f], keys[l])
        assert _prefix(keys[g], keys[g + 1]) == whole
        assert f == g or _prefix(keys[f], keys[g]) > whole
        assert g + 1 == l or _prefix(keys[g + 1], keys[l]) > whole
        assert f == 0 or _prefix(keys[f - 1], keys[f]) < whole
        assert l == n - 1 or _prefix(keys[l], keys[l + 1]) < whole
        assert i in (f, l)  # Karras: a node is numbered by one end of its range
        for c, (cf, cl) in ((int(t["left"][i]), (f, g)), (int(t["right"][i]), (g + 1, l))):  # the children tile the parent
            if c < 0:
                assert cf == cl == ~c
                leaf_seen[~c] += 1
            else:
                assert (int(t["first"][c]), int(t["last"][c])) == (cf, cl) and cf < cl
                node_seen[c] += 1
    assert (leaf_seen == 1).all() and (node_seen == 1).all()
    if name.startswith("equal"):
        assert L.tree_depth(t) == math.ceil(math.log2(n))  # lbvh.hip's header: duplicates form a balanced subtree


def test_radix_tree_by_hand():
    """Codes 1 1 4 5 5 5: the root splits 1 1 | 4 5 5 5 (bit 2 of the code), the right half 4 | 5 5 5 (bit 0), the three fives by their
    positions 3 4 5 = 011 | 100 101 (bit 2 of the position), then 4 | 5."""
    t = L.radix_tree(np.array([1, 1, 4, 5, 5, 5], np.uint32))
    assert t["first"].tolist() == [0, 0, 2, 3, 4] and t["last"].tolist() == [5, 1, 5, 5, 5]
    assert t["left"].tolist() == [1, ~0, ~2, ~3, ~4] and t["right"].tolist() == [2, ~1, 3, 4, ~5]
    assert t["bit"].tolist() == [34, 0, 32, 2, 0]


def test_node_boxes_are_exact_unions():
    rng = np.random.default_rng(3)
    v = rng.uniform(-2, 2, (77, 9)).astype(F)
    t = L.build(v)
    box, _ = L.tri_boxes(v)
    assert np.array_equal(t["leaf_box"], box[t["order"]])
    for i in range(76):
        ids = t["order"][t["first"][i]:t["last"][i] + 1]
        assert np.array_equal(t["box"][i, :3], box[ids, :3].min(0)) and np.array_equal(t["box"][i, 3:], box[ids, 3:].max(0))
    for i in range(76):  # and a parent's box is the union of its children's
        kids = [t["leaf_box"][~c] if c < 0 else t["box"][c] for c in (int(t["left"][i]), int(t["right"][i]))]
        assert np.array_equal(t["box"][i, :3], np.minimum(kids[0][:3], kids[1][:3]))
        assert np.array_equal(t["box"][i, 3:], np.maximum(kids[0][3:], kids[1][3:]))


# ---------------------------------------------------------------------------------------------- clusters and leaves

def _tri(x, y=0.0, z=0.0, s=0.1):
    return [x, y, z, x + s, y, z, x, y + s, z + s]


def test_leaf_rule_by_hand():
    """Two identical triangles: splitting costs a + a against 2a, no gain, one leaf. Two far apart: their union is far larger than
    both, two leaves. Area of a box 1 x 2 x 3 is 2 * (2 + 6 + 3) = 22."""
    assert L.box_area(F([0, 0, 0, 1, 2, 3])) == 22 and L.box_area(F([1, 0, 0, 0, 2, 3])) == 0
    assert L.leaf_partition(L.build(F([_tri(0), _tri(0)]))) == ([(0, 2)], [(0, 2)])
    assert L.leaf_partition(L.build(F([_tri(0), _tri(50)]))) == ([(0, 1), (1, 1)], [(0, 2)])
    # four coincident triangles and one far away: the pair rule applies at every level
    leaves, clusters = L.leaf_partition(L.build(F([_tri(0)] * 4 + [_tri(50)])))
    assert leaves == [(0, 4), (4, 1)] and clusters == [(0, 5)]
    # five coincident ones cannot be one leaf: the balanced subtree over positions 0..4 splits 0-3 | 4
    assert L.leaf_partition(L.build(F([_tri(0)] * 5)))[0] == [(0, 4), (4, 1)]


@pytest.mark.parametrize("n", [2, 5, 32, 33, 64, 65, 257, 1500])
def test_partition_invariants(n):
    rng = np.random.default_rng(n)
    v = (rng.uniform(-1, 1, (n, 1, 3)) + rng.uniform(-0.05, 0.05, (n, 3, 3))).astype(F).reshape(n, 9)
    if n == 1500:
        v[::3] = v[0]  # a third of the triangles coincide
    t = L.build(v)
    leaves, clusters = L.leaf_partition(t)
    for parts, cap in ((leaves, 4), (clusters, 32)):
        pos = 0
        for first, count in parts:
            assert first == pos and 1 <= count <= cap
            pos += count
        assert pos == n
    ranges = {(int(f), int(l) - int(f) + 1): i for i, (f, l) in enumerate(zip(t["first"], t["last"]))}
    parent = {}
    for i in range(n - 1):
        for c in (int(t["left"][i]), int(t["right"][i])):
            parent[c] = i
    for first, count in clusters:  # maximal: a cluster is a subtree, and its parent is too big
        c = ~first if count == 1 else ranges[first, count]
        assert c == 0 or int(t["last"][parent[c]]) - int(t["first"][parent[c]]) + 1 > 32
    ends = np.cumsum([c for _, c in clusters])
    for first, count in leaves:  # no leaf crosses a cluster
        k = int(np.searchsorted(ends, first, side="right"))
        assert first + count <= ends[k]
        assert count == 1 or (first, count) in ranges
    assert L.leaf_partition(t, cluster_tris=n)[1] == [(0, n)]


# ---------------------------------------------------------------------------------------------- mutations: every comparison can fail

def _ulp_up(a):
    return np.nextafter(a, F(np.inf))


def test_mutation_order_swapped():
    v = np.random.default_rng(1).uniform(-1, 1, (40, 9)).astype(F)
    t = L.build(v)
    assert L.tree_mismatches(t, {k: t[k].copy() for k in L.TREE_FIELDS}) == []
    bad = {k: t[k].copy() for k in L.TREE_FIELDS}
    bad["order"][[10, 11]] = bad["order"][[11, 10]]
    assert L.tree_mismatches(t, bad) == ["order"]


def test_mutation_leaf_ids(scenes, blobs):
    """Two triangles of different leaves exchanged in the triangle array: the same ranges, other leaves."""
    for layout in (2, 73):
        _, nodes, tris = blobs("tess_2k", layout)
        want = L.leaf_ids(layout, nodes, tris)
        assert sorted(i for leaf in want for i in leaf) == list(range(len(scenes["tess_2k"].tri_mat)))
        (fa, ca), (fb, _) = L.leaves_of(layout, nodes)[:2]
        assert fb == fa + ca
        rec = tris.copy().reshape(-1, 48)
        rec[[fa, fb]] = rec[[fb, fa]]
        assert L.leaves_of(layout, nodes) == L.leaves_of(layout, nodes.copy()) and L.leaf_ids(layout, nodes, rec.reshape(-1)) != want


def test_mutation_box_one_ulp():
    v = np.random.default_rng(2).uniform(-1, 1, (40, 9)).astype(F)
    t = L.build(v)
    for node, k in ((0, 3), (17, 0), (38, 5)):
        bad = {f: t[f].copy() for f in L.TREE_FIELDS}
        bad["box"][node, k] = _ulp_up(bad["box"][node, k])
        assert L.tree_mismatches(t, bad) == ["box"]
    bad = {f: t[f].copy() for f in L.TREE_FIELDS}
    bad["left"][5], bad["right"][5] = t["right"][5], t["left"][5]
    assert L.tree_mismatches(t, bad) == ["left", "right"]


def test_mutation_leaf_split(scenes, blobs):
    """A leaf of two or more triangles of a width-4 blob cut in two, the second half in a free slot of the same node: still every
    triangle in exactly one leaf, but not the same leaves."""
    info, nodes, tris = blobs("tess_2k", 4)
    want = L.leaves_of(4, nodes)
    slots = nodes.copy().view(np.int32).reshape(-1, 4, 8)
    done = False
    for i in range(len(slots)):
        refs = slots[i, :, 3]
        free = np.nonzero(refs == L.EMPTY)[0]
        big = [c for c in range(4) if refs[c] < 0 and refs[c] != L.EMPTY and ((~refs[c]) & 7) >= 1]
        if len(free) and big:
            c, e = big[0], free[0]
            first, count = (~refs[c]) >> 3, ((~refs[c]) & 7) + 1
            slots[i, e] = slots[i, c]
            slots[i, c, 3] = ~((first << 3) | 0)
            slots[i, e, 3] = ~(((first + 1) << 3) | (count - 2))
            done = True
            break
    assert done
    mutated = slots.view(np.uint8).reshape(-1)
    got = L.leaves_of(4, mutated)
    assert got != want and len(got) == len(want) + 1 and (first, 1) in got and (first + 1, count - 1) in got
    assert sum(c for _, c in got) == len(scenes["tess_2k"].tri_mat)
    assert L.info_mismatches(info, 4, nodes, tris, scenes["tess_2k"].verts) == []


@pytest.mark.parametrize("layout", LAYOUTS)
def test_mutation_info_off_by_one(scenes, blobs, layout):
    info, nodes, tris = blobs("soup_5k", layout)
    verts = scenes["soup_5k"].verts
    fields = ("n_nodes", "max_depth", "stack_need", "sah_cost", "node_bytes")
    for k, delta in (("stack_need", 1), ("stack_need", -1), ("max_depth", 1), ("n_nodes", 1), ("node_bytes", 64)):
        bad = types.SimpleNamespace(**{f: getattr(info, f) for f in fields})
        setattr(bad, k, getattr(bad, k) + delta)
        assert L.info_mismatches(bad, layout, nodes, tris, verts) == [k], (k, delta)
    bad = types.SimpleNamespace(**{f: getattr(info, f) for f in fields})
    bad.sah_cost = info.sah_cost * (1 + 3e-5)
    assert L.info_mismatches(bad, layout, nodes, tris, verts) == ["sah_cost"]
    # and the bytes: an inner ref redirected to a leaf shortens the walk
    refs_at = {2: 12, 4: 12}.get(layout, 16)
    cut = nodes.copy()
    cut[refs_at:refs_at + 4] = np.array([~((0 << 3) | 0)], np.int32).view(np.uint8)
    assert L.walk_info(layout, cut) != L.walk_info(layout, nodes)
