"""The bytes of a docs/SPEC.md §4.1 blob, given its topology and the vertices: a plain numpy statement that the four producers of node
boxes are held to — the host quantiser (bvh_build.cpp), the device packer of layout 68 (lbvh.hip), and the refit's k_refit_tris and
k_refit_level (refit.hip). Tests only: no device, no libptrt.

SPEC §4.3 promises that every builder "puts exact unions of the padded triangle boxes in the blob" and that a refitted blob "is a blob a
builder could have emitted for the new vertices". So once the topology is fixed — the refs of every slot, the slot order, the leaf ranges
and the id word of every triangle record — every other byte follows from the vertices and the materials:

- a triangle record is v0 | id, e1 = v1 - v0 | material, e2 = v2 - v0 | 0 in float32 (blob_rules.h tri_rows);
- a leaf child's box is the min / max over the padded boxes (tests/lbvh_ref.py tri_boxes) of its records, an inner child's box the min /
  max over that node's children, bottom-up. Minima and maxima are taken in record order and in slot order with blob_rules.h's rule_min /
  rule_max, as the refit takes them; the order could only show in the sign of a zero, and a padded coordinate is zero only for a vertex
  coordinate of exactly -+1e-6f;
- layouts 2 and 4 store these boxes: slot c = {lo.xyz, ref, hi.xyz, 0}. An empty slot is what bvh_build.cpp emit_blob writes: the whole
  slot memset to zero, then ref = 0x7fffffff. The refit does not touch empty slots, so after an update they must still hold exactly that;
- layouts 68, 72 and 73 quantise them per node and axis (SPEC §4.1, the comments of blob_rules.h quantize_node):
    origin    the minimum of the used children's lo, in slot order;
    exponent  starts at that of the smallest power of two s >= f32(ext / 255), ext = f32(max hi - origin), clamped to [1, 254]
              (1 for ext = 0). Found here from the bits of the quotient: its biased exponent, plus one unless its mantissa is zero;
    qlo       floor(f32(f32(lo_c - origin) / s)), clamped to [0, 255], then stepped down while the decode f32(qlo * s + origin) > lo_c;
    qhi       ceil likewise, stepped up while the decode < hi_c;
    the exponent is raised by one and the axis redone while any used child's decoded interval fails to enclose [lo_c, hi_c].
  The decode is a single float32 add of an exact product (q <= 255 times a power of two), as tests/ray_caster64.py _node_slots argues;
  that holds while 255 * s is finite, exponent <= 246, far beyond any scene here (2^100 times the unit box reaches 219). The header's
  last resort at exponent 254 (keep what fits) is not restated. Quantised bytes of empty slots are 0, byte 15 is 0, layout 68's pad words
  (bytes 56-63) and the upper 32 bytes of a 128-byte node are 0. Refs and slot order are the input's; layout 73 keeps its octant slots.

`expected_blob` reads a blob for its topology only; `blob_mismatches` names the first differing (node, slot, field)."""
import numpy as np

import lbvh_ref as L
from lbvh_ref import EMPTY, STRIDE, F, _rmax, _rmin

FAN = {2: 2, 4: 4, 68: 4, 72: 8, 73: 8}
QUANTISED = (68, 72, 73)
sah_expected = L.exact_sah


def _u8(a):
    return np.ascontiguousarray(np.asarray(a).reshape(-1).view(np.uint8))


def refs_of(width, nodes):
    """(n_nodes, fan) int32: the ref of every slot, empty ones included."""
    nodes = _u8(nodes)
    assert nodes.size % STRIDE[width] == 0
    n = FAN[width]
    w = nodes.view(np.int32).reshape(-1, STRIDE[width] // 4)
    return (w[:, 4:4 + n] if width in QUANTISED else w[:, 3:8 * n:8]).copy()


def expected_records(tris48, verts, tri_mat):
    """The 48-byte records for the ids the blob's records carry (row 0 .w): uint8, same size."""
    ids = L.blob_order(tris48)
    v = np.ascontiguousarray(verts, F).reshape(-1, 3, 3)[ids]
    rec = np.zeros((len(ids), 12), F)
    rec[:, 0:3], rec[:, 4:7], rec[:, 8:11] = v[:, 0], (v[:, 1] - v[:, 0]).astype(F), (v[:, 2] - v[:, 0]).astype(F)
    u = rec.view(np.uint32)
    u[:, 3] = ids
    u[:, 7] = 0 if tri_mat is None else np.ascontiguousarray(tri_mat, np.uint32)[ids]
    return rec.view(np.uint8).reshape(-1)


def levels_of(refs):
    """Lists of node indices by depth, root first; every node must be reached exactly once."""
    if len(refs) == 0:
        return []
    out, seen = [np.zeros(1, np.int64)], np.zeros(len(refs), np.int64)
    seen[0] = 1
    while True:
        r = refs[out[-1]].reshape(-1)
        nxt = r[(r >= 0) & (r != EMPTY)].astype(np.int64)
        if nxt.size == 0:
            break
        assert nxt.max() < len(refs)
        np.add.at(seen, nxt, 1)
        out.append(nxt)
    assert (seen == 1).all(), "a node out of reach or reached twice"
    return out


def child_boxes(width, nodes, tris48, verts):
    """(lo, hi, used): (n_nodes, fan, 3) float32 exact unions of padded triangle boxes per child slot, and which slots are used.
    Unused slots hold +inf / -inf."""
    refs = refs_of(width, nodes)
    m, n = refs.shape
    tb = L.tri_boxes(verts)[0][L.blob_order(tris48)]
    used = refs != EMPTY
    lo, hi = np.full((m, n, 3), np.inf, F), np.full((m, n, 3), -np.inf, F)
    leaf = refs < 0
    first, count = (~refs) >> 3, ((~refs) & 7) + 1
    for j in range(8):  # record j of every leaf that has one, in record order
        at = leaf & (count > j)
        if not at.any():
            break
        assert (first[at] + j).max() < len(tb)
        b = tb[first[at] + j]
        lo[at], hi[at] = _rmin(lo[at], b[:, :3]), _rmax(hi[at], b[:, 3:])
    nlo, nhi = np.full((m, 3), np.inf, F), np.full((m, 3), -np.inf, F)
    for idx in levels_of(refs)[::-1]:  # deepest level first: the inner children of this level are done
        r = refs[idx]
        inner = (r >= 0) & (r != EMPTY)
        clo, chi = lo[idx], hi[idx]
        clo[inner], chi[inner] = nlo[r[inner]], nhi[r[inner]]
        lo[idx], hi[idx] = clo, chi
        a, b = np.full((len(idx), 3), np.inf, F), np.full((len(idx), 3), -np.inf, F)
        for c in range(n):  # slot order; an unused slot's +-inf changes nothing
            a, b = _rmin(a, clo[:, c]), _rmax(b, chi[:, c])
        nlo[idx], nhi[idx] = a, b
    return lo, hi, used


def _scale(e):
    return (np.asarray(e, np.uint32) << np.uint32(23)).view(F)


def quantise(lo, hi, used):
    """The quantiser on m nodes at once. lo, hi: (m, n, 3) float32 child boxes, used: (m, n) bool.
    Returns origin (m, 3) float32, exponent (m, 3) uint8, qlo, qhi (m, 3, n) uint8 (0 for unused children)."""
    lo, hi, used = np.asarray(lo, F), np.asarray(hi, F), np.asarray(used, bool)
    m, n, _ = lo.shape
    u = np.repeat(used[:, None, :], 3, axis=1).reshape(m * 3, n)          # one row per (node, axis)
    a = np.where(u, lo.transpose(0, 2, 1).reshape(m * 3, n), F(np.inf))
    b = np.where(u, hi.transpose(0, 2, 1).reshape(m * 3, n), F(-np.inf))
    org, top = np.full(m * 3, np.inf, F), np.full(m * 3, -np.inf, F)
    for c in range(n):
        org, top = _rmin(org, a[:, c]), _rmax(top, b[:, c])
    none = ~(org <= top)                                                   # a node without children
    org, top = np.where(none, F(0), org), np.where(none, F(0), top)
    with np.errstate(all="ignore"):
        ext = (top - org).astype(F)
        bits = (ext / F(255)).astype(F).view(np.uint32)
    e = (bits >> np.uint32(23)).astype(np.int64) + ((bits & np.uint32(0x7FFFFF)) != 0)
    e = np.clip(np.where(ext > 0, e, 1), 1, 254)
    ql_out, qh_out = np.zeros((m * 3, n), np.uint8), np.zeros((m * 3, n), np.uint8)
    todo = np.arange(m * 3)
    while todo.size:
        s, o = _scale(e[todo])[:, None], org[todo][:, None]
        lo_c, hi_c, uc = np.where(u[todo], a[todo], o), np.where(u[todo], b[todo], o), u[todo]

        def dec(q):
            return ((q * s).astype(F) + o).astype(F)

        with np.errstate(all="ignore"):
            ql = np.clip(np.floor(((lo_c - o).astype(F) / s).astype(F)), 0, 255).astype(F)
            qh = np.clip(np.ceil(((hi_c - o).astype(F) / s).astype(F)), 0, 255).astype(F)
            while True:
                down = (ql > 0) & ~(dec(ql) <= lo_c)
                up = (qh < 255) & ~(dec(qh) >= hi_c)
                if not (down.any() or up.any()):
                    break
                ql, qh = ql - down.astype(F), qh + up.astype(F)
            fits = (((dec(ql) <= lo_c) & (dec(qh) >= hi_c)) | ~uc).all(axis=1)
        done = fits | (e[todo] >= 254)
        ql_out[todo[done]] = np.where(uc, ql, 0)[done].astype(np.uint8)
        qh_out[todo[done]] = np.where(uc, qh, 0)[done].astype(np.uint8)
        todo = todo[~done]
        e[todo] += 1
    return org.reshape(m, 3), e.reshape(m, 3).astype(np.uint8), ql_out.reshape(m, 3, n), qh_out.reshape(m, 3, n)


def pack_quantised(width, refs, org, ex, qlo, qhi):
    """Node bytes of layout 68 / 72 / 73 from the quantiser's output and the refs."""
    m, n = refs.shape
    out = np.zeros((m, STRIDE[width]), np.uint8)
    out[:, 0:12] = np.ascontiguousarray(org, F).view(np.uint8).reshape(m, 12)
    out[:, 12:15] = ex
    out[:, 16:16 + 4 * n] = np.ascontiguousarray(refs, np.int32).view(np.uint8).reshape(m, 4 * n)
    q0 = 16 + 4 * n
    out[:, q0:q0 + 3 * n] = qlo.reshape(m, 3 * n)
    out[:, q0 + 3 * n:q0 + 6 * n] = qhi.reshape(m, 3 * n)
    return out.reshape(-1)


def pack_f32(refs, lo, hi, used):
    """Node bytes of layout 2 / 4: {lo.xyz, ref, hi.xyz, 0} per used slot, {0, 0, 0, 0x7fffffff, 0, 0, 0, 0} per empty one."""
    m, n = refs.shape
    out = np.zeros((m, n, 8), F)
    out[:, :, 0:3], out[:, :, 4:7] = np.where(used[..., None], lo, F(0)), np.where(used[..., None], hi, F(0))
    out.view(np.int32)[:, :, 3] = refs
    return out.view(np.uint8).reshape(-1)


def expected_blob(width, nodes, tris48, verts, tri_mat):
    """(nodes_expected, tris_expected), uint8 arrays of the input's sizes. The input blob gives the topology only: the refs of every slot
    and the id word of every record."""
    assert width in FAN, width
    refs = refs_of(width, nodes)
    tris = expected_records(tris48, verts, tri_mat)
    assert tris.size == _u8(tris48).size
    if len(refs) == 0:
        return np.zeros(0, np.uint8), tris
    lo, hi, used = child_boxes(width, nodes, tris48, verts)
    if width in QUANTISED:
        return pack_quantised(width, refs, *quantise(lo, hi, used)), tris
    return pack_f32(refs, lo, hi, used), tris


def blob_mismatches(width, nodes, tris48, want_nodes, want_tris, limit=8):
    """The first `limit` differences between a blob and the expected bytes as (node, slot, field), nodes before records. field is one of
    'origin', 'exponent' (slot: the axis), 'ref', 'qlo', 'qhi', 'f32 box' (slot: the child slot), 'pad' (slot: None) and 'record'
    (node: the record's index, slot: its row). [] if every byte agrees."""
    got, want = _u8(nodes), _u8(want_nodes)
    gt, wt = _u8(tris48), _u8(want_tris)
    assert got.size == want.size and gt.size == wt.size and gt.size % 48 == 0, "blobs of different sizes"
    n, stride = FAN[width], STRIDE[width]
    bad = []
    diff = (got != want).reshape(-1, stride)
    for i in np.nonzero(diff.any(axis=1))[0].tolist():
        d = diff[i]
        if width in QUANTISED:
            q0 = 16 + 4 * n
            bad += [(i, k, "origin") for k in range(3) if d[4 * k:4 * k + 4].any()]
            bad += [(i, k, "exponent") for k in range(3) if d[12 + k]]
            bad += [(i, c, "ref") for c in range(n) if d[16 + 4 * c:20 + 4 * c].any()]
            bad += [(i, c, "qlo") for c in range(n) if d[q0 + c:q0 + 3 * n:n].any()]
            bad += [(i, c, "qhi") for c in range(n) if d[q0 + 3 * n + c:q0 + 6 * n:n].any()]
            if d[15] or d[q0 + 6 * n:].any():
                bad.append((i, None, "pad"))
        else:
            for c in range(n):
                s = d[32 * c:32 * c + 32]
                if s[0:12].any() or s[16:28].any():
                    bad.append((i, c, "f32 box"))
                if s[12:16].any():
                    bad.append((i, c, "ref"))
                if s[28:32].any():
                    bad.append((i, None, "pad"))
        if len(bad) >= limit:
            return bad[:limit]
    rd = (gt != wt).reshape(-1, 3, 16)
    for j in np.nonzero(rd.any(axis=(1, 2)))[0].tolist():
        bad += [(j, row, "record") for row in range(3) if rd[j, row].any()]
        if len(bad) >= limit:
            break
    return bad[:limit]
