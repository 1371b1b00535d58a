"""tests/blob_ref.py earns its trust without a device, before tests/test_gpu_blob_ref.py lets it judge the GPU builder and the refit.

The numpy statement is compared byte for byte with the host builder (the x86 build of blob_rules.h) on every scene and layout of
tests/golden/make_blob_digests.py; the quantiser is held to nodes worked out by hand at its edges; every field blob_mismatches can
name is shown to be reported when one byte of it moves — including the moves that pto_bvh_validate accepts, which is the gap these
tests close; and a blob whose boxes only ever grow (the stale box united with the new one) is shown to validate and to be caught."""
import dataclasses
import importlib.util
import os

import numpy as np
import pytest

import blob_ref as B
import lbvh_ref as L
from trace_support import LAYOUTS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_blob_digests", os.path.join(GOLDEN, "make_blob_digests.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

SCENES = ("cornell", "cornell_glass", "tess_2k", "tess_70k", "soup_5k", "soup_50k", "duplicates", "stacked_layers")
F = np.float32


@pytest.fixture(scope="module")
def scenes(P):
    sc = M.scenes(P)
    assert tuple(sc) == SCENES
    return sc


@pytest.fixture(scope="module")
def blobs(P, scenes):
    cache = {}

    def get(scene, layout):
        if (scene, layout) not in cache:
            info, nodes, tris = P.host.build_bvh_detached(scenes[scene], layout)
            cache[scene, layout] = (info, nodes.copy(), tris.copy())
        return cache[scene, layout]
    return get


# ---------------------------------------------------------------------------------------------- the host builder, byte for byte

@pytest.mark.parametrize("layout", M.LAYOUTS)
@pytest.mark.parametrize("scene", SCENES)
def test_host_blob_is_the_expected_blob(scenes, blobs, scene, layout):
    """expected_blob of a host blob's own topology is that blob: nodes and records, every byte. (Layout 0 is the default, 68 or 2.)"""
    info, nodes, tris = blobs(scene, layout)
    sd = scenes[scene]
    want_nodes, want_tris = B.expected_blob(info.width, nodes, tris, sd.verts, sd.tri_mat)
    assert want_nodes.dtype == np.uint8 and want_nodes.size == nodes.size and want_tris.size == tris.size
    assert B.blob_mismatches(info.width, nodes, tris, want_nodes, want_tris) == []
    assert np.array_equal(want_nodes, nodes) and np.array_equal(want_tris, tris)


def test_empty_blob_and_no_materials():
    n, t = B.expected_blob(68, np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros((0, 9), F), np.zeros(0, np.uint32))
    assert n.size == 0 and t.size == 0 and B.blob_mismatches(68, n, t, n, t) == []
    rec = np.zeros(12, np.uint32)
    rec[3] = 1  # one record, for triangle 1
    v = F([[9] * 9, [1, 2, 3, 2, 4, 6, 0, 0, 0]])
    got = B.expected_records(rec.view(np.uint8), v, None).view(F)
    assert got.tolist() == [1, 2, 3, got[3], 1, 2, 3, 0, -1, -2, -3, 0] and got.view(np.uint32)[3] == 1


# ---------------------------------------------------------------------------------------------- the quantiser by hand

def quantise_axis(intervals, n=4):
    """One node of n slots whose children have the given (lo, hi) on every axis (None: an empty slot). Returns (origin, exponent, qlo,
    qhi) of axis 0, after checking that the three axes agree."""
    lo, hi, used = np.zeros((1, n, 3), F), np.zeros((1, n, 3), F), np.zeros((1, n), bool)
    for c, iv in enumerate(intervals):
        if iv is not None:
            lo[0, c], hi[0, c], used[0, c] = F(iv[0]), F(iv[1]), True
    org, ex, qlo, qhi = B.quantise(lo, hi, used)
    assert org.shape == (1, 3) and ex.shape == (1, 3) and qlo.shape == (1, 3, n) and qhi.shape == (1, 3, n)
    for k in (1, 2):
        assert org[0, k].view(np.uint32) == org[0, 0].view(np.uint32) and ex[0, k] == ex[0, 0]
        assert np.array_equal(qlo[0, k], qlo[0, 0]) and np.array_equal(qhi[0, k], qhi[0, 0])
    return org[0, 0], int(ex[0, 0]), qlo[0, 0].tolist(), qhi[0, 0].tolist()


def decode(org, ex, q):
    return F(F(q) * B._scale(ex) + org)


def test_quantiser_extent_255_times_a_power_of_two():
    """Children [0, 1/2] and [1/4, 255/256]: ext / 255 = 2^-8 exactly, so s = 2^-8 (exponent 127 - 8 = 119), the grid's last step is the
    extent: qlo = 0, 64 and qhi = 128, 255. With the upper end one float higher, 255/256 + 2^-24, the quotient is 2^-8 + 2^-32 * 1.0039,
    just above the midpoint of 2^-8 and the next float 2^-8 + 2^-31: it rounds up, the smallest power of two above it is 2^-7
    (exponent 120), and qlo = 0, 32, qhi = 64, ceil(127.5 + 2^-17) = 128."""
    assert quantise_axis([(0, 0.5), (0.25, 255 / 256)]) == (0, 119, [0, 64, 0, 0], [128, 255, 0, 0])
    up = np.nextafter(F(255 / 256), F(2))
    assert up == F(255 / 256) + F(2.0 ** -24) and F(up / F(255)) == F(2.0 ** -8) + F(2.0 ** -31)
    assert quantise_axis([(0, 0.5), (0.25, up)]) == (0, 120, [0, 32, 0, 0], [64, 128, 0, 0])
    # the same at another power of two, 255 * 2^20
    assert quantise_axis([(0, 2.0 ** 27), (2.0 ** 26, 255 * 2.0 ** 20)]) == (0, 147, [0, 64, 0, 0], [128, 255, 0, 0])


def test_quantiser_axis_with_only_the_padding():
    """The z axis of the `planar` scene of tests/blob_scenes.py: every vertex at z = -0.5, every child [-0.5 - pad, -0.5 + pad] with
    pad = 1e-6f. Floats are 2^-24 apart above 0.5 in magnitude and 2^-25 below: lo = -(0.5 + 17 * 2^-24) (1e-6 = 16.8 * 2^-24),
    hi = -(0.5 - 34 * 2^-25) (1e-6 = 33.6 * 2^-25), ext = 34 * 2^-24 = 17 * 2^-23 exactly. ext / 255 = 2^-23 / 15 lies between 2^-27 and
    2^-26: s = 2^-26, exponent 101, qlo = 0, qhi = 17 * 8 = 136, whose decode is hi exactly."""
    box, _ = L.tri_boxes(F([[0, 0, -0.5, 1, 0, -0.5, 0, 1, -0.5]]))
    lo, hi = box[0, 2], box[0, 5]
    assert lo == -(F(0.5) + F(17 * 2.0 ** -24)) and hi == -(F(0.5) - F(17 * 2.0 ** -24))
    org, ex, qlo, qhi = quantise_axis([(lo, hi)] * 4)
    assert (org, ex, qlo, qhi) == (lo, 101, [0] * 4, [136] * 4) and decode(org, ex, 136) == hi


def test_quantiser_one_used_child_and_empty_slots():
    """One child [1, 3] in slot 2: origin 1, 2 / 255 = 2^-7 * 1.0039, s = 2^-6 (121), qhi = 2 * 64 = 128; empty slots are 0.
    Eight slots with 1, 4 and 7 empty, children [0,1] [1,2] [2,3] [3,4] [7,8]: 8 / 255 = 2^-5 * 1.0039, s = 2^-4 (123), q = 16 x."""
    assert quantise_axis([None, None, (1, 3), None]) == (1, 121, [0, 0, 0, 0], [0, 0, 128, 0])
    assert quantise_axis([(0, 1), None, (1, 2), (2, 3), None, (3, 4), (7, 8), None], n=8) == \
        (0, 123, [0, 0, 16, 32, 0, 48, 112, 0], [16, 0, 32, 48, 0, 64, 128, 0])


def test_pack_quantised_by_hand():
    """The bytes of the two layouts for the eight-slot node above (x), a scaled copy on y and z, and of a four-slot node: origin,
    exponents, byte 15, refs, the six coordinate groups of N bytes with child c in byte c, zero padding behind them."""
    iv = [(0, 1), None, (1, 2), (2, 3), None, (3, 4), (7, 8), None]
    lo, hi, used = np.zeros((1, 8, 3), F), np.zeros((1, 8, 3), F), np.zeros((1, 8), bool)
    for c, v in enumerate(iv):
        if v:
            lo[0, c], hi[0, c], used[0, c] = F(v[0]) * F([1, 2, 4]) - F([0, 1, 0]), F(v[1]) * F([1, 2, 4]) - F([0, 1, 0]), True
    refs = np.array([[5, B.EMPTY, ~8, 6, B.EMPTY, ~((3 << 3) | 2), 7, B.EMPTY]], np.int32)
    raw = B.pack_quantised(72, refs, *B.quantise(lo, hi, used))
    assert raw.size == 128 and raw[0:12].view(F).tolist() == [0, -1, 0] and raw[12:16].tolist() == [123, 124, 125, 0]
    assert np.array_equal(raw[16:48].view(np.int32), refs[0])
    ql, qh = [0, 0, 16, 32, 0, 48, 112, 0], [16, 0, 32, 48, 0, 64, 128, 0]
    assert raw[48:72].tolist() == ql * 3 and raw[72:96].tolist() == qh * 3 and not raw[96:].any()
    raw4 = B.pack_quantised(68, refs[:, :4], *B.quantise(lo[:, :4], hi[:, :4], used[:, :4]))  # children [0,1] - [1,2] [2,3]: 3/255 -> 2^-6
    assert raw4.size == 64 and raw4[12:16].tolist() == [121, 122, 123, 0] and np.array_equal(raw4[16:32].view(np.int32), refs[0, :4])
    assert raw4[32:44].tolist() == [0, 0, 64, 128] * 3 and raw4[44:56].tolist() == [64, 0, 128, 192] * 3 and not raw4[56:].any()


def test_quantiser_negative_origin_and_signed_zero():
    """[-3, -1] and [-2.5, 0.5]: origin -3, 3.5 / 255 = 2^-7 * 1.757, s = 2^-6 (121), qlo = 0, 32, qhi = 128, 224.
    Lower ends +0.0 and -0.0: the origin is the first of them in slot order (rule_min keeps what it has unless the other is smaller,
    and neither zero is smaller), either way q = 0 for both and 1 / 255 gives s = 2^-7 (120), qhi = 128."""
    assert quantise_axis([(-3, -1), (-2.5, 0.5)]) == (-3, 121, [0, 32, 0, 0], [128, 224, 0, 0])
    for first, second in ((0.0, -0.0), (-0.0, 0.0)):
        org, ex, qlo, qhi = quantise_axis([(first, 1), (second, 1)])
        assert org.view(np.uint32) == F(first).view(np.uint32) and (ex, qlo, qhi) == (120, [0] * 4, [128, 128, 0, 0])


NEAR = {  # origin: spacing of float32 there
    1e4: 2.0 ** -10, -1e4: 2.0 ** -10, 1e6: 2.0 ** -4,
}


@pytest.mark.parametrize("origin", sorted(NEAR))
def test_quantiser_extent_of_a_few_float_spacings(origin):
    """Children [o, o + 2u] and [o + u, o + 3u] with u the spacing of floats at o (2^-10 at 1e4, 2^-4 at 1e6; at -1e4 the node runs
    towards zero, where floats are as dense or denser). ext = 3u, 3 / 255 = 2^-7 * 1.506, so s = u * 2^-6: the grid is 64 times finer
    than the floats it has to decode to. Every coordinate sits on a multiple of u = 64 s, qlo = 0, 64 and qhi = 128, 192, and those decode
    to the coordinates exactly (q * s + o is a float, the add does not round), so the start exponent holds: where the differences
    lo_c - origin are exact, floor and ceil already enclose and a finer grid than the floats costs nothing. The node scaled by 2^-30,
    2^30 and 2^100: the same bytes, the exponent moved by the power."""
    u = NEAR[origin]
    o = F(origin)
    assert np.nextafter(o, F(np.inf)) - o == F(u)
    iv = [(o, o + F(2 * u)), (o + F(u), o + F(3 * u))]
    e0 = 127 + int(np.log2(u)) - 6
    assert quantise_axis(iv) == (o, e0, [0, 64, 0, 0], [128, 192, 0, 0])
    for c, (a, b) in enumerate(iv):
        assert decode(o, e0, [0, 64][c]) == a and decode(o, e0, [128, 192][c]) == b
    for k in (-30, 30, 100):
        s = F(2.0 ** k)
        assert quantise_axis([(a * s, b * s) for a, b in iv]) == (o * s, e0 + k, [0, 64, 0, 0], [128, 192, 0, 0])


def test_quantiser_widens_when_the_extent_rounds_down():
    """The widening loop by hand. One child [-255, 2^-30]: ext = f32(2^-30 + 255) = 255, the subtraction rounds the small end away,
    s = 1 (127) and qhi = ceil(255 / 1) = 255 decodes to 0 < 2^-30 with no step left: the exponent goes to 128, s = 2,
    qhi = ceil(127.5) = 128 decodes to 1. Next to a child that ends at 0 exactly, which s = 1 would have fitted."""
    tiny = F(2.0 ** -30)
    assert F(tiny - F(-255)) == 255
    assert quantise_axis([(-255, tiny)]) == (-255, 128, [0, 0, 0, 0], [128, 0, 0, 0])
    assert quantise_axis([(-255, 0)]) == (-255, 127, [0, 0, 0, 0], [255, 0, 0, 0])
    assert quantise_axis([(-255, 0), (-100.5, tiny)]) == (-255, 128, [0, 77, 0, 0], [128, 128, 0, 0])


def test_quantiser_steps_after_an_inexact_difference():
    """The two stepping loops by hand. Children [-1000, 0.75] and [4 - 2^-21, 8 + 2^-20]: ext = f32(1008 + 2^-20) = 1008, / 255 = 3.95,
    s = 4 (129). Floats near 1000 are 2^-14 apart, so the second child's lo - origin = 1004 - 2^-21 rounds up to 1004: floor(251) = 251
    decodes to 4 > lo, one step down to 250 (decode 0). Its hi - origin = 1008 + 2^-20 rounds down to 1008: ceil(252) decodes to
    8 < hi, one step up to 253 (decode 12). The first child: qlo = 0, qhi = ceil(1000.75 / 4 = 250.19) = 251."""
    lo1, hi1 = F(4) - F(2.0 ** -21), F(8) + F(2.0 ** -20)
    assert lo1 < 4 and hi1 > 8 and F(lo1 - F(-1000)) == 1004 and F(hi1 - F(-1000)) == 1008
    assert quantise_axis([(-1000, 0.75), (lo1, hi1)]) == (-1000, 129, [0, 250, 0, 0], [251, 253, 0, 0])
    assert decode(F(-1000), 129, 250) == 0 and decode(F(-1000), 129, 253) == 12


@pytest.mark.parametrize("layout", (68, 72, 73))
def test_quantised_blobs_decode_to_enclosing_boxes(scenes, blobs, layout):
    """The promise of SPEC §4.1 on the reference's own output, with the decoder of tests/ray_caster64.py: every decoded box encloses the
    exact union it stands for, and by less than two grid steps per side."""
    import ray_caster64 as rc
    sd = scenes["soup_5k"]
    _, nodes, tris = blobs("soup_5k", layout)
    want, _ = B.expected_blob(layout, nodes, tris, sd.verts, sd.tri_mat)
    lo, hi, used = B.child_boxes(layout, nodes, tris, sd.verts)
    for i in range(0, len(lo), 7):
        slots = rc._node_slots(layout, want, i)
        sc = B._scale(want[i * B.STRIDE[layout] + 12:i * B.STRIDE[layout] + 15]).astype(np.float64)
        cs = np.nonzero(used[i])[0]
        assert len(slots) == len(cs)
        for (dlo, dhi, _), c in zip(slots, cs):
            assert (dlo <= lo[i, c]).all() and (dhi >= hi[i, c]).all()
            assert (lo[i, c] - dlo < 2 * sc).all() and (dhi - hi[i, c] < 2 * sc).all()


# ---------------------------------------------------------------------------------------------- mutations: every comparison can fail

def _validates(pto, sd, width, nodes, tris):
    return pto.Scene(sd, (width, np.ascontiguousarray(nodes), np.ascontiguousarray(tris))).validate_bvh()[0] == 0


def _pick(nodes, n, want):
    """(node, slot, axis) of the first used slot of a BVH4Q / BVH8Q blob for which want(node bytes, slot, axis) holds."""
    stride = 64 if n == 4 else 128
    raw = nodes.reshape(-1, stride)
    for i in range(len(raw)):
        refs = raw[i, 16:16 + 4 * n].view(np.int32)
        for c in range(n):
            for a in range(3):
                if refs[c] != B.EMPTY and want(raw[i], c, a):
                    return i, c, a
    raise AssertionError("no such slot")


@pytest.mark.parametrize("layout", (68, 72))
def test_mutations_of_a_quantised_blob(pto, scenes, blobs, layout):
    """On the host's blob of the tessellated scene: one qlo byte - 1, one qhi byte + 1, one exponent + 1 with that axis's bytes halved
    outward, the origin one float lower with that axis's bytes re-derived, a nonzero pad word. blob_mismatches names node, slot and
    field of each, and the oracle's structural check accepts the four that still enclose: it cannot see them."""
    sd = scenes["tess_2k"]
    _, nodes, tris = blobs("tess_2k", layout)
    n = B.FAN[layout]
    q0, stride = 16 + 4 * n, B.STRIDE[layout]
    want = B.expected_blob(layout, nodes, tris, sd.verts, sd.tri_mat)
    assert B.blob_mismatches(layout, nodes, tris, *want) == [] and _validates(pto, sd, layout, nodes, tris)

    def check(mut, expect, encloses=True):
        assert B.blob_mismatches(layout, mut, tris, *want, limit=64) == expect
        if encloses:
            assert _validates(pto, sd, layout, mut, tris), expect

    i, c, a = _pick(nodes, n, lambda nd, c, a: nd[q0 + a * n + c] > 0)
    mut = nodes.copy()
    mut[i * stride + q0 + a * n + c] -= 1
    check(mut, [(i, c, "qlo")])

    i, c, a = _pick(nodes, n, lambda nd, c, a: nd[q0 + (3 + a) * n + c] < 255)
    mut = nodes.copy()
    mut[i * stride + q0 + (3 + a) * n + c] += 1
    check(mut, [(i, c, "qhi")])

    i, a = len(nodes) // stride // 2, 1  # a node in the middle, axis y: a grid twice as coarse, floor(qlo / 2) and ceil(qhi / 2)
    mut = nodes.copy()
    nd = mut[i * stride:(i + 1) * stride]
    used = nd[16:16 + 4 * n].view(np.int32) != B.EMPTY
    nd[12 + a] += 1
    lo_at, hi_at = slice(q0 + a * n, q0 + a * n + n), slice(q0 + (3 + a) * n, q0 + (3 + a) * n + n)
    old_lo, old_hi = nd[lo_at].copy(), nd[hi_at].copy()
    nd[lo_at], nd[hi_at] = old_lo // 2, (old_hi.astype(int) + 1) // 2
    moved = [(i, int(c), "qlo") for c in np.nonzero(used & (nd[lo_at] != old_lo))[0]] + [(i, int(c), "qhi") for c in np.nonzero(used & (nd[hi_at] != old_hi))[0]]
    assert moved
    check(mut, [(i, a, "exponent")] + moved)

    # the origin one float lower: every decoded coordinate of the axis moves down with it, so the bytes are taken again (the largest
    # q that decodes to <= lo, the smallest that decodes to >= hi) on a node where they still fit
    lo, hi, _ = B.child_boxes(layout, nodes, tris, sd.verts)
    for i in range(len(lo)):
        a = 2
        nd = nodes[i * stride:(i + 1) * stride]
        used = nd[16:16 + 4 * n].view(np.int32) != B.EMPTY
        org = np.nextafter(nd[4 * a:4 * a + 4].view(F)[0], F(-np.inf))
        grid = decode(org, nd[12 + a], np.arange(256))
        ql = [int(np.nonzero(grid <= lo[i, c, a])[0].max(initial=-1)) if used[c] else 0 for c in range(n)]
        qh = [int(np.nonzero(grid >= hi[i, c, a])[0].min(initial=256)) if used[c] else 0 for c in range(n)]
        if min(ql) >= 0 and max(qh) <= 255:
            break
    else:
        raise AssertionError("no node takes an origin one float lower")
    mut = nodes.copy()
    nd = mut[i * stride:(i + 1) * stride]
    nd[4 * a:4 * a + 4] = np.array([org], F).view(np.uint8)
    old_lo, old_hi = nd[q0 + a * n:q0 + a * n + n].copy(), nd[q0 + (3 + a) * n:q0 + (3 + a) * n + n].copy()
    nd[q0 + a * n:q0 + a * n + n], nd[q0 + (3 + a) * n:q0 + (3 + a) * n + n] = ql, qh
    moved = [(i, c, "qlo") for c in range(n) if ql[c] != old_lo[c]] + [(i, c, "qhi") for c in range(n) if qh[c] != old_hi[c]]
    check(mut, [(i, a, "origin")] + moved)

    for at in ((60, 15) if layout == 68 else (96, 127, 15)):  # a pad word, and the byte next to the exponents
        mut = nodes.copy()
        mut[5 * stride + at] = 1
        check(mut, [(5, None, "pad")], encloses=False)


@pytest.mark.parametrize("layout", (2, 4))
def test_mutations_of_an_f32_blob(pto, scenes, blobs, layout):
    """One box one ulp wider (still encloses: the structural check accepts it), the zero word of a slot set, an empty slot's box
    bytes set."""
    sd = scenes["tess_2k"]
    _, nodes, tris = blobs("tess_2k", layout)
    want = B.expected_blob(layout, nodes, tris, sd.verts, sd.tri_mat)
    assert B.blob_mismatches(layout, nodes, tris, *want) == []
    for node, slot, word in ((0, 0, 4), (7, 1, 0), (len(nodes) // (32 * layout) - 1, 0, 6)):
        mut = nodes.copy()
        f = mut.view(F).reshape(-1, layout, 8)
        assert f.view(np.int32)[node, slot, 3] != B.EMPTY
        f[node, slot, word] = np.nextafter(f[node, slot, word], F(np.inf if word >= 4 else -np.inf))
        assert B.blob_mismatches(layout, mut, tris, *want) == [(node, slot, "f32 box")]
        assert _validates(pto, sd, layout, mut, tris)
    mut = nodes.copy()
    mut.view(np.uint32).reshape(-1, layout, 8)[3, 1, 7] = 1
    assert B.blob_mismatches(layout, mut, tris, *want) == [(3, None, "pad")]
    if layout == 4:
        refs = B.refs_of(layout, nodes)
        node, slot = [int(x[0]) for x in np.nonzero(refs == B.EMPTY)]
        assert not nodes.view(np.uint32).reshape(-1, layout, 8)[node, slot, [0, 1, 2, 4, 5, 6, 7]].any()  # what emit_blob leaves there
        mut = nodes.copy()
        mut.view(F).reshape(-1, layout, 8)[node, slot, 5] = 1.0
        assert B.blob_mismatches(layout, mut, tris, *want) == [(node, slot, "f32 box")]


def test_mutations_of_the_records(pto, scenes, blobs):
    """e1 one ulp off, a material word, the zero word: named by record and row. Two records exchanged change the topology (the id
    words), so the expected blob follows them and the difference shows in the boxes of the leaves that hold them."""
    sd = scenes["tess_2k"]
    _, nodes, tris = blobs("tess_2k", 68)
    want = B.expected_blob(68, nodes, tris, sd.verts, sd.tri_mat)
    for rec, word, row in ((0, 5, 1), (1234, 9, 2), (len(tris) // 48 - 1, 0, 0)):
        mut = tris.copy()
        f = mut.view(F).reshape(-1, 12)
        f[rec, word] = np.nextafter(f[rec, word], F(np.inf))
        assert B.blob_mismatches(68, nodes, mut, *want) == [(rec, row, "record")]
        assert not _validates(pto, sd, 68, nodes, mut)  # the structural check compares the records with the vertices: it sees this one
    for rec, word, row in ((17, 7, 1), (18, 11, 2)):
        mut = tris.copy()
        mut.view(np.uint32).reshape(-1, 12)[rec, word] ^= 1
        assert B.blob_mismatches(68, nodes, mut, *want) == [(rec, row, "record")]
    (fa, ca), (fb, _) = L.leaves_of(68, nodes)[:2]
    mut = tris.copy().reshape(-1, 48)
    mut[[fa, fb]] = mut[[fb, fa]]
    bad = B.blob_mismatches(68, nodes, mut.reshape(-1), *B.expected_blob(68, nodes, mut.reshape(-1), sd.verts, sd.tri_mat))
    assert bad and all(f in ("origin", "exponent", "qlo", "qhi") for _, _, f in bad)


def test_mismatches_are_limited_and_sizes_checked(scenes, blobs):
    sd = scenes["tess_2k"]
    _, nodes, tris = blobs("tess_2k", 72)
    want = B.expected_blob(72, nodes, tris, sd.verts, sd.tri_mat)
    bad = B.blob_mismatches(72, np.zeros_like(nodes), np.zeros_like(tris), *want)
    assert len(bad) == 8 and bad[0][0] == 0
    assert len(B.blob_mismatches(72, nodes, np.zeros_like(tris), *want, limit=3)) == 3
    with pytest.raises(AssertionError):
        B.blob_mismatches(72, nodes[:-128], tris, *want)


# ---------------------------------------------------------------------------------------------- the refit that only grows

def shrunk_to_leaves(width, nodes, tris, verts):
    """Every triangle pulled half way towards the centre of its leaf's vertices: every box of the tree gets smaller."""
    v = np.ascontiguousarray(verts, F).reshape(-1, 3, 3).astype(np.float64)
    ids = L.blob_order(tris)
    out = v.copy()
    for first, count in L.leaves_of(width, nodes):
        mine = ids[first:first + count]
        centre = v[mine].reshape(-1, 3).mean(0)
        out[mine] = centre + 0.5 * (v[mine] - centre)
    return out.astype(F).reshape(-1, 9)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_grow_only_refit_validates_and_is_caught(pto, scenes, blobs, layout):
    """The negative control for the refit tests. Vertices A are the scene's, B pulls every triangle towards its leaf's centre. A refit
    that unites each new box with the stale one leaves, per slot, the union of A's and B's exact boxes (quantised for the Q layouts) next
    to B's records. That blob passes the structural check against B — and so every check the suite had — and differs from
    expected_blob(B) in most nodes."""
    sd = scenes["tess_2k"]
    _, nodes, tris = blobs("tess_2k", layout)
    vb = shrunk_to_leaves(layout, nodes, tris, sd.verts)
    sb = dataclasses.replace(sd, verts=vb)
    want_nodes, want_tris = B.expected_blob(layout, nodes, tris, vb, sd.tri_mat)
    assert _validates(pto, sb, layout, want_nodes, want_tris)
    assert not np.array_equal(want_nodes, nodes) and not np.array_equal(want_tris, tris)
    (alo, ahi, used), (blo, bhi, _) = B.child_boxes(layout, nodes, tris, sd.verts), B.child_boxes(layout, nodes, tris, vb)
    lo, hi = np.minimum(alo, blo), np.maximum(ahi, bhi)
    assert (blo[used] >= alo[used]).mean() > 0.9 and (lo[used] < blo[used]).any()  # B's boxes lie inside A's, nearly everywhere
    refs = B.refs_of(layout, nodes)
    grown = B.pack_quantised(layout, refs, *B.quantise(lo, hi, used)) if layout in B.QUANTISED else B.pack_f32(refs, lo, hi, used)
    assert _validates(pto, sb, layout, grown, want_tris)
    bad = B.blob_mismatches(layout, grown, want_tris, want_nodes, want_tris, limit=10 ** 6)
    assert len({i for i, _, _ in bad}) > len(refs) // 2, len(bad)
    assert all(f in ("origin", "exponent", "qlo", "qhi", "f32 box") for _, _, f in bad)
