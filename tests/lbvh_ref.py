"""What the GPU BVH builder (pathtracing_amd/csrc/lbvh.hip, PT_BVH_BUILD_LBVH) promises, restated in numpy and plain Python. Tests only:
no device, no libptrt.

Written from docs/SPEC.md §4.1 and §4.3, the header comments of lbvh.hip and bvh_build.cpp and the rules of blob_rules.h, with other
algorithms than the kernels use wherever the promise leaves room:

- the Morton code is interleaved bit by bit (the kernel spreads bits with multiplies);
- the radix tree is built top-down over the augmented 64-bit keys `code << 32 | position`, splitting every range at the highest bit
  in which its first and last key differ (the kernel finds every node's range bottom-up by binary searches on common-prefix
  lengths). Karras's numbering falls out of the split: a left child that is an inner node carries the index of its last leaf, a
  right child that of its first leaf, the root is 0 — so left / right / first / last compare elementwise with k_hierarchy's arrays;
- a node's box is the min / max over the slice of sorted triangle boxes under its range (the kernel walks up from the leaves);
- clusters and leaves are found by walking down from the root (k_mark decides per node from its parent).

Float32 throughout where the library computes in float32, in the library's operation order (-ffp-contract=off, correctly rounded
divide), so that codes, order, boxes, areas and the leaf rule agree bit for bit.

The second half checks any SPEC §4.1 blob from its bytes, on all five layouts: `walk_info`, `exact_sah`, `leaves_of`, `blob_order`.
Nodes are decoded with tests/ray_caster64.py `_node_slots`.
"""
from bisect import bisect_left

import numpy as np

import ray_caster64 as rc

F = np.float32
EMPTY = 0x7FFFFFFF
STRIDE = {2: 64, 4: 128, 68: 64, 72: 128, 73: 128}


# ---------------------------------------------------------------------------------------------- triangle boxes, codes, order

def _rmin(a, b):  # blob_rules.h rule_min: b < a ? b : a
    return np.where(b < a, b, a)


def _rmax(a, b):  # blob_rules.h rule_max: a < b ? b : a
    return np.where(a < b, b, a)


def tri_boxes(verts):
    """(boxes (n, 6) float32: padded lo xyz, hi xyz; centroids (n, 3) float32) — blob_rules.h tri_box."""
    v = np.ascontiguousarray(verts, F).reshape(-1, 3, 3)
    lo = _rmin(v[:, 0], _rmin(v[:, 1], v[:, 2]))
    hi = _rmax(v[:, 0], _rmax(v[:, 1], v[:, 2]))

    def pad(c):
        return (F(1e-6) * _rmax(np.ones_like(c), np.abs(c))).astype(F)

    box = np.concatenate([(lo - pad(lo)).astype(F), (hi + pad(hi)).astype(F)], axis=1)
    cent = (F(0.5) * (lo + hi).astype(F)).astype(F)
    return box, cent


def quantise_centroids(cent):
    """(n, 3) uint32 grid coordinates in [0, 1023]: (c - cmin) * inv * 1024 in float32, clamped with fmax / fmin semantics (a NaN from
    0 * inf maps to 0), truncated. inv = 1 / (cmax - cmin), or 0 on an axis without extent."""
    cent = np.ascontiguousarray(cent, F).reshape(-1, 3)
    lo, hi = cent.min(0), cent.max(0)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        ext = (hi - lo).astype(F)
        inv = np.where(hi > lo, (F(1) / np.where(hi > lo, ext, F(1))).astype(F), F(0)).astype(F)
        x = (((cent - lo).astype(F) * inv).astype(F) * F(1024)).astype(F)
    x = np.where(np.isnan(x), F(0), x)            # fmaxf(NaN, 0) = 0
    x = np.where(x > F(0), x, F(0))               # fmaxf(x, 0)
    x = np.where(x < F(1023), x, F(1023))         # fminf(x, 1023); +inf -> 1023
    return x.astype(np.uint32)                    # truncation (x >= 0)


def morton_codes(cent):
    """30-bit Morton codes of the centroids: 10 bits per axis, interleaved x y z from the top (bit 29 = x's bit 9)."""
    q = quantise_centroids(cent)
    code = np.zeros(len(q), np.uint32)
    for b in range(10):
        for axis in range(3):
            code |= ((q[:, axis] >> np.uint32(b)) & np.uint32(1)) << np.uint32(3 * b + 2 - axis)
    return code


def sort_order(codes):
    """Triangle index of every sorted position: the stable sort by code (a radix sort whose values start as the identity)."""
    return np.argsort(np.asarray(codes, np.uint32), kind="stable").astype(np.uint32)


# ---------------------------------------------------------------------------------------------- the binary radix tree

def radix_tree(codes_sorted):
    """The binary radix tree over the keys (code, position), for n >= 2 sorted codes. Returns a dict of arrays of n - 1 inner nodes in
    Karras's numbering: left, right (int32: >= 0 inner node, < 0 leaf ~position), first, last (uint32: the node's range, inclusive),
    split (the last position of the left child) and bit (the bit of the 64-bit key the node splits at)."""
    codes = [int(c) for c in np.asarray(codes_sorted)]
    n = len(codes)
    assert n >= 2 and all(codes[i] <= codes[i + 1] for i in range(n - 1))
    keys = [(c << 32) | i for i, c in enumerate(codes)]
    left, right = np.zeros(n - 1, np.int32), np.zeros(n - 1, np.int32)
    first, last = np.zeros(n - 1, np.uint32), np.zeros(n - 1, np.uint32)
    split, bit = np.zeros(n - 1, np.uint32), np.zeros(n - 1, np.int32)
    seen = np.zeros(n - 1, bool)
    todo = [(0, 0, n - 1)]  # (node index, first, last)
    while todo:
        i, f, l = todo.pop()
        assert not seen[i]
        seen[i] = True
        b = (keys[f] ^ keys[l]).bit_length() - 1            # the highest bit in which the range's keys differ
        g = bisect_left(keys, (keys[l] >> b) << b, f, l + 1) - 1  # keys[f .. g] have that bit clear, keys[g + 1 .. l] have it set
        assert f <= g < l
        first[i], last[i], split[i], bit[i] = f, l, g, b
        if f == g:
            left[i] = ~g
        else:
            left[i] = g
            todo.append((g, f, g))
        if g + 1 == l:
            right[i] = ~(g + 1)
        else:
            right[i] = g + 1
            todo.append((g + 1, g + 1, l))
    assert seen.all()
    return dict(left=left, right=right, first=first, last=last, split=split, bit=bit)


def tree_depth(tree):
    """Edges from the root to the deepest leaf."""
    best, todo = 0, [(0, 0)]
    while todo:
        i, d = todo.pop()
        for c in (int(tree["left"][i]), int(tree["right"][i])):
            if c < 0:
                best = max(best, d + 1)
            else:
                todo.append((c, d + 1))
    return best


def node_boxes(tree, sorted_boxes):
    """(n - 1, 6) float32: per inner node the exact union of the padded triangle boxes under its range."""
    sb = np.ascontiguousarray(sorted_boxes, F)
    out = np.empty((len(tree["first"]), 6), F)
    for i, (f, l) in enumerate(zip(tree["first"].tolist(), tree["last"].tolist())):
        out[i, :3] = sb[f:l + 1, :3].min(0)
        out[i, 3:] = sb[f:l + 1, 3:].max(0)
    return out


def build(verts):
    """The whole reference for one triangle array: dict with order, codes (sorted), left, right, first, last, box, leaf_box (sorted)."""
    box, cent = tri_boxes(verts)
    codes = morton_codes(cent)
    order = sort_order(codes)
    t = radix_tree(codes[order])
    t["order"], t["codes"], t["leaf_box"] = order, codes[order], box[order]
    t["box"] = node_boxes(t, t["leaf_box"])
    return t


TREE_FIELDS = ("order", "left", "right", "first", "last", "box")


def tree_mismatches(want, got):
    """Names of the fields of TREE_FIELDS in which two trees differ in shape, type or any bit."""
    bad = []
    for k in TREE_FIELDS:
        a, b = np.ascontiguousarray(want[k]), np.ascontiguousarray(got[k])
        if a.dtype != b.dtype or a.size != b.size or not np.array_equal(a.reshape(-1).view(np.uint32), b.reshape(-1).view(np.uint32)):
            bad.append(k)
    return bad


# ---------------------------------------------------------------------------------------------- clusters and leaves

def box_area(b):
    """blob_rules.h Box::area in float32: 0 for an empty box, else 2 * ((dx * dy + dy * dz) + dz * dx)."""
    b = np.asarray(b, F)
    dx, dy, dz = F(b[3] - b[0]), F(b[4] - b[1]), F(b[5] - b[2])
    if dx < 0:
        return F(0)
    return F(F(2) * F(F(F(dx * dy) + F(dy * dz)) + F(dz * dx)))


def leaf_partition(tree, cluster_tris=32, max_leaf=4):
    """(leaves, clusters): sorted lists of (first, count) over the sorted positions. Clusters: the maximal subtrees of at most
    `cluster_tris` triangles. Inside a cluster a subtree of at most `max_leaf` triangles is one leaf unless splitting it lowers the SAH
    cost, area(left) * count(left) + area(right) * count(right) < area(node) * count(node), in float32."""
    left, right, first, last = tree["left"], tree["right"], tree["first"], tree["last"]

    def count(c):
        return 1 if c < 0 else int(last[c]) - int(first[c]) + 1

    def start(c):
        return ~c if c < 0 else int(first[c])

    def area(c):
        return box_area(tree["leaf_box"][~c] if c < 0 else tree["box"][c])

    clusters, todo = [], [0]
    while todo:
        c = todo.pop()
        if c < 0 or count(c) <= cluster_tris:
            clusters.append(c)
        else:
            todo += [int(left[c]), int(right[c])]
    leaves, todo = [], list(clusters)
    while todo:
        c = todo.pop()
        if c < 0:
            leaves.append((~c, 1))
            continue
        kids = (int(left[c]), int(right[c]))
        if count(c) <= max_leaf:
            split = F(F(area(kids[0]) * F(count(kids[0]))) + F(area(kids[1]) * F(count(kids[1]))))
            if not split < F(area(c) * F(count(c))):
                leaves.append((int(first[c]), count(c)))
                continue
        todo += kids
    return sorted(leaves), sorted((start(c), count(c)) for c in clusters)


# ---------------------------------------------------------------------------------------------- checkers of a blob's bytes

def _nodes_u8(nodes):
    return np.ascontiguousarray(np.asarray(nodes).reshape(-1).view(np.uint8))


def _refs(width, nodes):
    """Per node the list of its used slots' refs, in slot order."""
    nodes = _nodes_u8(nodes)
    assert nodes.size % STRIDE[width] == 0
    return [[r for _, _, r in rc._node_slots(width, nodes, i)] for i in range(nodes.size // STRIDE[width])]


def _leaf(ref):
    return (~ref) >> 3, ((~ref) & 7) + 1


def _postorder(refs):
    """Inner nodes reachable from node 0, children before parents; every node at most once (a second visit is a malformed blob)."""
    if not refs:
        return []
    out, seen, todo = [], set(), [0]
    while todo:
        i = todo.pop()
        assert 0 <= i < len(refs) and i not in seen, f"node {i} out of range or reached twice"
        seen.add(i)
        out.append(i)
        todo += [r for r in refs[i] if r >= 0]
    return out[::-1]


def walk_info(width, nodes):
    """(nodes reachable from the root, max_depth, stack_need) from a blob's bytes, by the conventions of bvh_build.cpp emit_blob and
    lbvh.hip k_depth: a node's depth is 1 + the largest depth of its inner children, which counts as 1 without any; its need is (used
    slots - 1) + the largest need of its inner children. No nodes: (0, 0, 0)."""
    refs = _refs(width, nodes)
    depth, need = {}, {}
    for i in _postorder(refs):
        inner = [r for r in refs[i] if r >= 0]
        depth[i] = 1 + max([1] + [depth[r] for r in inner])
        need[i] = max(len(refs[i]) - 1, 0) + max([0] + [need[r] for r in inner])
    return (len(depth), depth[0], need[0]) if refs else (0, 0, 0)


def leaves_of(width, nodes):
    """Sorted (first, count) of every leaf reachable from the root."""
    refs = _refs(width, nodes)
    return sorted(_leaf(r) for i in _postorder(refs) for r in refs[i] if r < 0)


def blob_order(tris48):
    """The original triangle ids of a blob's 48-byte triangles, in array order."""
    return np.ascontiguousarray(_nodes_u8(tris48)).view(np.uint32).reshape(-1, 12)[:, 3].copy()


def leaf_ids(width, nodes, tris48):
    """Sorted list of the leaves as tuples of original triangle ids, in the order the leaf holds them: what a blob's leaves are
    whatever order the packer emitted them in (the host packer emits leaves breadth-first, docs/SPEC.md §4.1)."""
    ids = blob_order(tris48).tolist()
    return sorted(tuple(ids[f:f + c]) for f, c in leaves_of(width, nodes))


def partition_ids(tree, leaves):
    """The reference's leaves (first, count over the sorted positions) as sorted tuples of triangle ids, to compare with leaf_ids."""
    order = np.asarray(tree["order"]).tolist()
    return sorted(tuple(order[f:f + c]) for f, c in leaves)


def exact_sah(width, nodes, tris48, verts):
    """pt_bvh_info.sah_cost from the bytes and the scene's vertices (SPEC §4.3): every child's exact float32 union box is recomputed from
    the padded boxes of the triangles under it — not decoded from the node —, and the sum over child slots of f32(area / root area), times
    the triangle count for a leaf, is taken in float64. The root area is that of all triangles' union, at least 1e-30."""
    refs = _refs(width, nodes)
    if not refs:
        return 0.0
    tb = tri_boxes(verts)[0][blob_order(tris48)]
    lo, hi = {}, {}  # per inner node: the union of its children

    def child_box(r):
        if r >= 0:
            return lo[r], hi[r]
        f, c = _leaf(r)
        return tb[f:f + c, :3].min(0), tb[f:f + c, 3:].max(0)

    slots = []  # (box6, leaf count or 1)
    for i in _postorder(refs):
        boxes = [child_box(r) for r in refs[i]]
        lo[i] = np.min([b[0] for b in boxes], axis=0)
        hi[i] = np.max([b[1] for b in boxes], axis=0)
        slots += [(np.concatenate(b), _leaf(r)[1] if r < 0 else 1) for b, r in zip(boxes, refs[i])]
    root = max(box_area(np.concatenate([lo[0], hi[0]])), F(1e-30))
    return float(sum(float(F(box_area(b) / root)) * k for b, k in slots))


def numpy_sah(nodes, width):
    """bvh_build.cpp emit_blob's cost restated on the stored f32 slots of layouts 2 and 4 (tests/test_gpu_update.py holds the refit to it;
    exact_sah extends it to the quantised layouts): sum of f32(area / root area) (times the count for a leaf), in float64."""
    n = width
    slots = np.frombuffer(nodes.tobytes(), np.float32).reshape(-1, n, 8)
    refs = slots[:, :, 3].view(np.int32)
    lo, hi = slots[:, :, 0:3], slots[:, :, 4:7]

    def area(lo, hi):
        d = (hi - lo).astype(np.float32)
        a = np.float32(2) * (d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0])
        return np.where(d[..., 0] < 0, np.float32(0), a).astype(np.float32)

    used = refs != 0x7FFFFFFF
    rlo, rhi = lo[0][used[0]].min(0), hi[0][used[0]].max(0)
    ra = np.maximum(area(rlo, rhi), np.float32(1e-30))
    cnt = np.where(refs < 0, (~refs & 7) + 1, 1).astype(np.float64)
    q = (area(lo, hi) / ra).astype(np.float32).astype(np.float64)
    return float((q * cnt)[used].sum())


def info_mismatches(info, width, nodes, tris48, verts, rtol=1e-5):
    """Names of the fields of a pt_bvh_info (anything with n_nodes, max_depth, stack_need, sah_cost, node_bytes) that disagree with the
    blob's bytes: the three integers exactly, node_bytes = n_nodes * stride, sah_cost within `rtol` of exact_sah."""
    reach, depth, need = walk_info(width, nodes)
    bad = [k for k, a, b in (("n_nodes", info.n_nodes, reach), ("max_depth", info.max_depth, depth), ("stack_need", info.stack_need, need),
                             ("node_bytes", info.node_bytes, reach * STRIDE[width])) if int(a) != int(b)]
    if _nodes_u8(nodes).size != reach * STRIDE[width]:
        bad.append("unreachable nodes")
    sah = exact_sah(width, nodes, tris48, verts)
    if not abs(float(info.sah_cost) - sah) <= rtol * sah:
        bad.append("sah_cost")
    return bad
