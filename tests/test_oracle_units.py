"""Unit and analytic checks of the scalar oracle (docs/SPEC.md). The reference has none of this,
so these are self-consistency and physics checks, not reference parity."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from trace_support import LAYOUTS

HERE = os.path.dirname(os.path.abspath(__file__))
F3 = C.c_float * 3


def _pcg(x):
    """SPEC §2 in Python integers: every product and sum is reduced mod 2^32 where u32 arithmetic wraps."""
    m = 0xFFFFFFFF
    s = (x * 747796405 + 2891336453) & m
    w = (((s >> ((s >> 28) + 4)) ^ s) * 277803737) & m
    return (w >> 22) ^ w


def _pcg_inverse(y):
    """The x with pcg(x) == y: pcg is a bijection of u32 (an odd multiplier and an xorshift by at least 4 each way)."""
    m = 0xFFFFFFFF
    w = y ^ (y >> 22)                                   # the shift is more than half the word: one step undoes it
    v = (w * pow(277803737, -1, 1 << 32)) & m
    r = (v >> 28) + 4                                   # the top four bits of s pass through s ^ (s >> r) unchanged
    s = v
    for _ in range(8):                                  # each step settles r more bits from the top
        s = v ^ (s >> r)
    return ((s - 2891336453) * pow(747796405, -1, 1 << 32)) & m


def _path_key(seed, pixel, sample):
    return _pcg((_pcg((_pcg(seed) + pixel) & 0xFFFFFFFF) + sample) & 0xFFFFFFFF)


def _rnd(key, dim):
    return _pcg((key + dim * 0x9E3779B9) & 0xFFFFFFFF)


def _u01(key, dim):
    return np.float32(_rnd(key, dim) >> 8) * np.float32(2.0 ** -24)  # a 24-bit integer and its product with 2^-24 are exact in f32


def test_rng_stream(pto):
    """pto_pcg, pto_path_key and pto_u01 against SPEC §2 restated in Python integers, on the edges of u32: seed, pixel and sample of 0,
    1, 2^31 and 2^32 - 1 (the sums pcg(..) + pixel and .. + sample wrap), every dimension a path of 255 segments and a lens draw, and a
    few beyond (dim * 0x9E3779B9 wraps from dim = 2 on); u01 stays below 1 at the largest rnd."""
    edge = (0, 1, 1 << 31, 0xFFFFFFFF)
    for x in edge + (2, 0x7FFFFFFF, 0x80000001, 0x5EED0001, 129708002):
        assert pto.lib.pto_pcg(x) == _pcg(x), x
    keys = set()
    for seed in edge:
        for pixel in edge:
            for sample in edge:
                k = _path_key(seed, pixel, sample)
                assert pto.lib.pto_path_key(seed, pixel, sample) == k, (seed, pixel, sample)
                keys.add(k)
    assert len(keys) == 64  # pcg is a bijection of u32 and every stage adds its argument: distinct triples, distinct keys
    # the sums wrap: a pixel of 2^32 - 1 is a pixel of -1
    assert _path_key(5, 0xFFFFFFFF, 7) == _pcg((_pcg((_pcg(5) - 1) & 0xFFFFFFFF) + 7) & 0xFFFFFFFF)
    dims = list(range(1026 + 3 * 254 + 1)) + [1 << 16, (1 << 31) - 1, 1 << 31, 0xFFFFFFFE, 0xFFFFFFFF]
    for key in (0, 1, 0xFFFFFFFF, _path_key(0x5EED0001, 12345, 7)):
        for dim in dims:
            got = np.float32(pto.lib.pto_u01(key, dim))
            assert got == _u01(key, dim) and 0.0 <= got < 1.0, (key, dim, got)
    # the largest rnd: 2^32 - 1 >> 8 = 2^24 - 1, times 2^-24, is the largest float below 1
    top = np.float32(0xFFFFFFFF >> 8) * np.float32(2.0 ** -24)
    assert top == np.float32(1.0) - np.float32(2.0 ** -24) and top < 1.0 and np.nextafter(top, np.float32(2.0)) == np.float32(1.0)
    for r in (0xFFFFFFFF, 0xFFFFFF00, 0xFFFFFEFF, 0):  # keys whose dimension 0, and whose dimension 3, draw exactly r
        x = _pcg_inverse(r)
        assert _pcg(x) == r and pto.lib.pto_pcg(x) == r
        want = top if r >= 0xFFFFFF00 else np.float32(r >> 8) * np.float32(2.0 ** -24)
        assert np.float32(pto.lib.pto_u01(x, 0)) == want < 1.0, r
        assert np.float32(pto.lib.pto_u01((x - 3 * 0x9E3779B9) & 0xFFFFFFFF, 3)) == want, r
    k = pto.lib.pto_path_key(0x5EED0001, 12345, 7)
    assert k == pto.lib.pto_path_key(0x5EED0001, 12345, 7)
    assert k != pto.lib.pto_path_key(0x5EED0001, 12346, 7) and k != pto.lib.pto_path_key(0x5EED0001, 12345, 8)
    u = np.array([pto.lib.pto_u01(k, d) for d in range(4096)], np.float64)
    assert (u >= 0).all() and (u < 1).all()
    assert abs(u.mean() - 0.5) < 0.03 and abs(u.var() - 1 / 12) < 0.01
    # counter based: value depends on (key, dim) only
    assert pto.lib.pto_u01(k, 17) == pto.lib.pto_u01(k, 17)


def test_sincos2pi(pto):
    s, c = C.c_float(), C.c_float()
    us = np.concatenate([np.linspace(0, 1, 4001, endpoint=False), [0.25, 0.5, 0.75, 1 - 2.0 ** -24]]).astype(np.float32)
    err = 0.0
    for u in us:
        pto.lib.pto_sincos2pi(float(u), C.byref(s), C.byref(c))
        err = max(err, abs(s.value - np.sin(2 * np.pi * float(u))), abs(c.value - np.cos(2 * np.pi * float(u))))
    assert err < 5e-7


def _mat(P, kind, albedo, rough=0.0, ior=1.5, emission=(0, 0, 0)):
    m = np.zeros(1, P.MATERIAL_DTYPE)
    m["kind"], m["albedo"], m["emission"], m["roughness"], m["ior"] = kind, albedo, emission, rough, ior
    return m


def _sample(pto, m, d, n, front, u):
    wi, W, side = F3(), F3(), C.c_float()
    alive = pto.lib.pto_bsdf_sample(m.ctypes.data_as(C.c_void_p), F3(*d), F3(*n), front, u[0], u[1], u[2], wi, W, C.byref(side))
    return alive, np.array(wi[:]), np.array(W[:]), side.value


@pytest.mark.parametrize("kind,rough", [(0, 0.0), (1, 0.0), (1, 0.3), (1, 1.0), (2, 0.0)])
def test_bsdf_energy_and_geometry(P, pto, kind, rough):
    rng = np.random.default_rng(1)
    m = _mat(P, kind, (0.9, 0.8, 0.7), rough)
    n = np.array([0.0, 0.0, 1.0], np.float32)
    for _ in range(2000):
        d = rng.normal(size=3); d[2] = -abs(d[2]) - 1e-3; d /= np.linalg.norm(d)
        alive, wi, W, side = _sample(pto, m, d.astype(np.float32), n, 1, rng.random(3).astype(np.float32))
        if not alive:
            continue
        assert abs(np.linalg.norm(wi) - 1) < 1e-5
        assert (W >= 0).all() and (W <= 1.0 + 1e-5).all()        # no BSDF sample amplifies energy
        assert np.sign(wi[2]) == side                              # reflect stays above n, transmit goes below
        if kind == 1 and rough == 0.0:
            np.testing.assert_allclose(wi, d - 2 * np.dot(d, n) * n, atol=2e-6)


def test_lambert_is_cosine_weighted(P, pto):
    m = _mat(P, 0, (1, 1, 1))
    n = np.array([0.3, -0.5, 0.81], np.float32); n /= np.linalg.norm(n)
    rng = np.random.default_rng(2)
    cs = []
    for _ in range(20000):
        _, wi, _, _ = _sample(pto, m, -n, n, 1, rng.random(3).astype(np.float32))
        cs.append(float(np.dot(wi, n)))
    cs = np.array(cs)
    assert (cs >= -1e-6).all()
    assert abs(cs.mean() - 2 / 3) < 0.01          # E[cos] under a cosine-weighted pdf
    assert abs((cs ** 2).mean() - 0.5) < 0.01


def test_dielectric_normal_incidence_fresnel(P, pto):
    m = _mat(P, 2, (1, 1, 1), ior=1.5)
    n = np.array([0, 0, 1], np.float32); d = np.array([0, 0, -1], np.float32)
    refl = sum(_sample(pto, m, d, n, 1, np.array([0, 0, u], np.float32))[3] > 0 for u in np.linspace(0, 1, 1000, endpoint=False))
    assert refl in (40, 41)                        # F0 = ((1.5-1)/(1.5+1))^2 = 0.04
    # Snell at 45 degrees entering glass
    d = np.array([np.sin(np.pi / 4), 0, -np.cos(np.pi / 4)], np.float32)
    _, wi, _, side = _sample(pto, m, d, n, 1, np.array([0, 0, 0.99], np.float32))
    assert side == -1 and abs(np.hypot(wi[0], wi[1]) - np.sin(np.pi / 4) / 1.5) < 1e-6
    # total internal reflection from inside
    d = np.array([np.sin(1.0), 0, -np.cos(1.0)], np.float32)
    _, wi, _, side = _sample(pto, m, d, n, 0, np.array([0, 0, 0.99], np.float32))
    assert side == 1


def test_furnace(P, pto):
    """White-furnace: a Lambert sphere of albedo a under a uniform sky of radiance 1 has expected radiance
    sum_k a^k * P(escape at k); with a = 1 and RR every path carries exactly the sky => image == 1 wherever finite."""
    sd = P.SceneData()
    sd.spheres = np.array([[0, 0, 0, 1.0]], np.float32); sd.sph_mat = np.zeros(1, np.uint32)
    sd.mats = _mat(P, 0, (1, 1, 1)); sd.sky = np.ones(3, np.float32)
    sd.cam = P.make_scene(0, 0, 1, 64, 64).cam
    p = P.make_params(64, 64, spp=16, max_depth=64, rr_start=200)
    img, st = pto.render(pto.Scene(sd), p)
    assert np.allclose(img[..., :3], 1.0, atol=1e-5), (img[..., :3].min(), img[..., :3].max())
    # with RR on, still unbiased: mean stays 1 within noise
    p.rr_start = 2; p.max_depth = 200
    img2, _ = pto.render(pto.Scene(sd), p)
    assert abs(img2[..., :3].mean() - 1.0) < 0.01


def test_oracle_bvh_equals_brute_force(P, pto):
    sd = P.make_scene(P.native.PT_SCENE_TRIANGLE_SOUP, 3000, 7, 96, 96)
    p = P.make_params(96, 96, spp=2, max_depth=4)
    brute, st0 = pto.render(pto.Scene(sd), p)
    s = pto.Scene(sd); s.build_own_bvh(); assert s.validate_bvh()[0] == 0
    fast, st1 = pto.render(s, p)
    assert st0.rays == st1.rays and np.array_equal(brute, fast)  # the (t, prim id) rule makes the hit structure-independent
    assert st1.tri_tests < st0.tri_tests / 20


@pytest.mark.parametrize("kind,detail", [(0, 0), (1, 0), (2, 5000), (3, 4000)])
@pytest.mark.parametrize("width", LAYOUTS)
def test_product_bvh_blob_validates_and_matches_brute_force(P, pto, kind, detail, width):
    """The product's host-side builder (detached scene, no device) against the oracle's structural validator, and the
    oracle traversing those bytes against brute force."""
    from pathtracing_amd.host import build_bvh_detached
    sd = P.make_scene(kind, detail, 3, 64, 64)
    info, nodes, tris = build_bvh_detached(sd, width)
    assert info.width == width and info.n_tris == len(sd.tri_mat) and info.node_bytes == info.n_nodes * (64 if width == 68 else 128 if width in (72, 73) else width * 32)
    s = pto.Scene(sd, (width, nodes, tris))
    rc, depth = s.validate_bvh()
    assert rc == 0 and depth == info.max_depth
    p = P.make_params(64, 64, spp=1, max_depth=3)
    a, sa = pto.render(s, p)
    b, sb = pto.render(pto.Scene(sd), p)
    assert sa.rays == sb.rays and np.array_equal(a, b)


def test_validator_rejects_corruption(P, pto):
    from pathtracing_amd.host import build_bvh_detached
    sd = P.make_scene(2, 500, 3, 64, 64)
    info, nodes, tris = build_bvh_detached(sd, 2)
    bad = tris.copy(); bad[12] ^= 0x40                      # flip a bit in a triangle's orig id
    assert pto.Scene(sd, (2, nodes, bad)).validate_bvh()[0] != 0
    bad = nodes.copy().view(np.float32); bad[0] += 0.5      # shrink a root child box
    assert pto.Scene(sd, (2, bad.view(np.uint8), tris)).validate_bvh()[0] != 0


def test_c1_golden_pin(P, pto):
    pin = json.load(open(os.path.join(HERE, "golden", "c1_cornell_oracle.json")))
    sd = P.make_scene(P.native.PT_SCENE_CORNELL, 0, 0x5EED0001, 256, 256)
    p = P.make_params(256, 256, spp=4, max_depth=8, rr_start=3, seed=0x5EED0001)
    img, st = pto.render(pto.Scene(sd), p)
    assert st.rays == pin["rays"] and st.paths == pin["paths"]
    assert hashlib.sha256(np.ascontiguousarray(img).tobytes()).hexdigest() == pin["sha256_f32"]
    assert (img[..., 3] == 1.0).all()


def test_sample_streams_in_the_oracle(P, pto):
    """SPEC §5: K partial sums per pixel. K = 0/1 is the plain sequential sum; other K only reassociate float additions."""
    sd = P.make_scene(0, 0, 1, 48, 48)
    a, sa = pto.render(pto.Scene(sd), P.make_params(48, 48, spp=9, max_depth=5, streams=1))
    z, _ = pto.render(pto.Scene(sd), P.make_params(48, 48, spp=9, max_depth=5, streams=0))
    assert np.array_equal(a, z)
    for k in (2, 4, 16, 64):
        b, sb = pto.render(pto.Scene(sd), P.make_params(48, 48, spp=9, max_depth=5, streams=k))
        assert sb.rays == sa.rays and np.abs(a - b).max() < 2e-6 and (b[..., 3] == 1).all()
    with pytest.raises(RuntimeError):
        pto.render(pto.Scene(sd), P.make_params(48, 48, spp=2, streams=65))


def test_threads_do_not_change_the_image(P, pto):
    sd = P.make_scene(0, 0, 1, 48, 48)
    p = P.make_params(48, 48, spp=2, max_depth=5)
    a, _ = pto.render(pto.Scene(sd), p, threads=1)
    b, _ = pto.render(pto.Scene(sd), p, threads=4)
    assert np.array_equal(a, b)


def test_default_layout_follows_scene_size(P, pto):
    """PT_BVH_WIDTH_DEFAULT: BVH2 (float boxes) for scenes of at most 192 triangles (the whole tree is a few L1-resident lines and the
    2-wide visit is the cheapest), BVH4Q above.
    Either way the blob validates and the oracle traversing it equals brute force (the quantised slab test of SPEC §4.1)."""
    from pathtracing_amd.host import build_bvh_detached
    for kind, detail, want in ((P.native.PT_SCENE_CORNELL, 0, 2), (P.native.PT_SCENE_CORNELL_TESS, 150, 2), (P.native.PT_SCENE_CORNELL_TESS, 3000, 68)):
        sd = P.make_scene(kind, detail, 5, 48, 48)
        info, nodes, tris = build_bvh_detached(sd, 0)
        assert info.width == want, (len(sd.tri_mat), info.width)
        s = pto.Scene(sd, (info.width, nodes, tris))
        assert s.validate_bvh()[0] == 0
        p = P.make_params(48, 48, spp=2, max_depth=4)
        a, sa = pto.render(s, p)
        b, sb = pto.render(pto.Scene(sd), p)
        assert sa.rays == sb.rays and np.array_equal(a, b)


def test_quantised_slab_test_is_conservative_on_grazing_rays(P, pto):
    """SPEC §4.1 folds the dequantisation into the slab test. Rays that graze box faces and run along axes (zero direction
    components, origins on node planes) are where a non-conservative plane would lose a hit: every layout must return
    exactly the brute-force closest hit."""
    from pathtracing_amd.host import build_bvh_detached
    sd = P.make_scene(P.native.PT_SCENE_CORNELL_TESS, 5000, 11, 32, 32)
    rng = np.random.default_rng(7)
    v = sd.verts.reshape(-1, 3, 3)
    rays = []
    for _ in range(300):
        t = v[rng.integers(len(v))]
        target = t[0] if rng.random() < 0.5 else (t[0] + t[1]) * 0.5          # a vertex or an edge midpoint
        o = np.array([0.0, 0.0, 0.0], np.float32) + rng.uniform(-0.3, 0.3, 3).astype(np.float32)
        if rng.random() < 0.3:
            o[rng.integers(3)] = target[rng.integers(3)]                       # origin in an axis plane of the target
        d = (target - o).astype(np.float32)
        if rng.random() < 0.3:
            d[rng.integers(3)] = 0.0                                           # axis-parallel component
        n = float(np.linalg.norm(d))
        if n > 1e-6:
            rays.append((o, (d / n).astype(np.float32)))
    brute = pto.Scene(sd)
    for width in LAYOUTS:
        info, nodes, tris = build_bvh_detached(sd, width)
        s = pto.Scene(sd, (width, nodes, tris))
        for o, d in rays:
            assert s.closest(o, d) == brute.closest(o, d)


def test_octant_slots_order_children_front_to_back(P, pto):
    """Layout 73 (BVH8O, docs/SPEC.md §4.1): the same 8-wide tree as layout 72, every child in the slot that names its corner of the
    node, visited in the order slot ^ ray octant with no distance sort. The order must be nearly as good as the sorted one: node
    visits within 2 % of layout 72's on a deep incoherent scene (an 8-wide tree visited in plain slot order needs more than twice as
    many), same pictures, same triangles, and far fewer visits than the 4-wide tree."""
    from pathtracing_amd.host import build_bvh_detached
    sd = P.make_scene(P.native.PT_SCENE_TRIANGLE_SOUP, 60000, 5, 96, 64)
    p = P.make_params(96, 64, spp=2, max_depth=6)
    res = {}
    for width in (68, 72, 73):
        info, nodes, tris = build_bvh_detached(sd, width)
        img, st = pto.render(pto.Scene(sd, (width, nodes, tris)), p)
        res[width] = (img, st, info, nodes)
    assert np.array_equal(res[72][0], res[73][0]) and np.array_equal(res[68][0], res[73][0])
    assert res[72][2].n_nodes == res[73][2].n_nodes and res[72][2].max_depth == res[73][2].max_depth  # the same tree, other slots
    v4, v8s, v8o = (res[k][1].node_visits for k in (68, 72, 73))
    assert v8o <= 1.02 * v8s and v8o < 0.8 * v4, (v4, v8s, v8o)
    # the two blobs are the same nodes with the same numbers of children (numbered in another order, since numbering follows the slots)
    a = np.frombuffer(res[72][3].tobytes(), "<i4").reshape(-1, 32)[:, 4:12]
    b = np.frombuffer(res[73][3].tobytes(), "<i4").reshape(-1, 32)[:, 4:12]
    assert np.array_equal(np.sort((a != 0x7FFFFFFF).sum(1)), np.sort((b != 0x7FFFFFFF).sum(1)))
    assert ((a != 0x7FFFFFFF).sum(1) < 8).any() and (b[(b != 0x7FFFFFFF).sum(1) < 8][:, 0] == 0x7FFFFFFF).any()  # 8O leaves holes anywhere, also in slot 0


def test_threaded_sah_build_is_the_serial_tree(P):
    """The host builder builds the subtrees below depth 4 on threads (bvh_build.cpp build_parallel): the blob must be the serial one,
    byte for byte. The serial reference comes from a child process pinned to one CPU (std::thread::hardware_concurrency() == 1)."""
    import hashlib, subprocess, sys, textwrap
    if len(os.sched_getaffinity(0)) < 2:
        pytest.skip("one CPU: the build is serial anyway")
    code = textwrap.dedent("""
        import os, sys, hashlib
        if sys.argv[1] == "serial": os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})
        sys.path.insert(0, %r)
        import numpy as np
        import pathtracing_amd as P
        from pathtracing_amd.host import build_bvh_detached
        for kind, detail in ((P.native.PT_SCENE_TRIANGLE_SOUP, 90000), (P.native.PT_SCENE_CORNELL_TESS, 120000)):
            sd = P.make_scene(kind, detail, 11, 32, 32)
            for width in (68, 2):
                info, nodes, tris = build_bvh_detached(sd, width)
                print(info.n_nodes, info.max_depth, info.stack_need, hashlib.md5(np.asarray(nodes).tobytes() + np.asarray(tris).tobytes()).hexdigest())
        """) % os.path.dirname(HERE)
    outs = [subprocess.run([sys.executable, "-c", code, mode], capture_output=True, text=True, timeout=600) for mode in ("serial", "threads")]
    assert all(o.returncode == 0 for o in outs), outs[0].stderr[-500:] + outs[1].stderr[-500:]
    assert outs[0].stdout == outs[1].stdout and len(outs[0].stdout.splitlines()) == 4
