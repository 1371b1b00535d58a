"""-m gpu: pt_gather and pt_gather_paths (docs/SPEC.md §12, §12.1) where the gather kernels had not run: trees whose traversal stack
spills into the overflow columns, the geometry space of tests/geometry_space.py, refitted geometry, batches of more than one grid
(the second pass of the kernels' grid-stride loop) and the u32 wrap of the key sums.

Every comparison is bit for bit (gather_device.call, bits, same): the eight floats of every record, and pt_stats::rays of
pt_gather_paths. The reference is the scalar checker of tests/gather_paths_ref/ on a pto.Scene of the same scene data, which
tests/test_gather_space.py holds to gather_ref and to float64 on these inputs. pt_gather is held to it through §12.1: its visibility
word and bent row are the checker's for every max_distance, and its whole record is the checker's with max_depth 1 and max_distance 0
on the scene without emitters — pt_gather never reads an emission, so that holds for its record on the lit scene too, which the tests
that cannot commit a second scene (a refit, the large batches) use.

K = 64 and the case's own ray_eps unless a test says otherwise; the translate cases, whose own ray_eps (1e-4 of the offset) carries
every origin out of the box, also run with gather_ref.tight_eps (tests/test_gather_space.py has the figures)."""
import dataclasses

import numpy as np
import pytest

import env_checker
import gather_paths_checker as GP
import gather_ref as G
import geometry_space
from gather_device import K, LBVH, SENTINEL, SKY, bits, call, same
from trace_support import LAYOUTS

pytestmark = pytest.mark.gpu

DEPTHS = ((8, 3), (2, 3))
GRID = 16384  # kTraceBlocks: the most one-wave workgroups of a launch


class Refs:
    """The checker's answers for one point set on one scene, made once and compared with the device on every layout: the lit scene at
    DEPTHS, and the scene without emitters at max_depth 1 for max_distance 0 and about half the scene's extent."""

    def __init__(self, pto, sd, pts, nrm, eps, env=None, depths=DEPTHS, **kw):
        self.lit = dataclasses.replace(sd, sky=SKY) if env is None else dataclasses.replace(sd, sky=SKY, environment=env)
        self.dark = GP.without_emission(self.lit)
        self.pts, self.nrm, self.eps, self.env, self.kw = pts, nrm, eps, env, kw
        self.osc, self.dosc = pto.Scene(self.lit), pto.Scene(self.dark)
        self.osc.build_own_bvh()
        self.dosc.build_own_bvh()
        self.rec = G.records(pts, nrm)
        self.valid = int(sum(G.valid_point(p, n) for p, n in zip(pts, nrm)))
        self.paths = {d: GP.gather(self.osc, pts, nrm, env=env, ray_eps=eps, max_depth=d[0], rr_start=d[1], **kw) for d in depths}
        self.sky = {md: GP.gather(self.dosc, pts, nrm, env=env, ray_eps=eps, max_depth=1, rr_start=0, max_distance=md, **kw)
                    for md in (0.0, G.half_box(sd))}

    def hold(self, P, r, ctx, host=True, lit=True):
        """Both calls on the committed scene (lit: the lit one) against the checker; returns every output, for the next layout."""
        outs = []
        for (md, rr), ref in self.paths.items() if lit else ():
            out, st = call(P, r, self.rec, host=host, ray_eps=self.eps, max_depth=md, rr_start=rr, **self.kw)
            bad = np.nonzero((bits(out) != bits(ref.rows)).any(1))[0]
            assert len(bad) == 0, (ctx, "paths", md, len(bad), bad[:4], out[bad[:2]], ref.rows[bad[:2]])
            assert st.rays == ref.rays and st.paths == len(self.rec), (ctx, "paths", md, st.rays, ref.rays, st.paths)
            outs.append(out)
        for dist, ref in self.sky.items():
            out, st = call(P, r, self.rec, host=host, paths=False, ray_eps=self.eps, max_distance=dist, **self.kw)
            bad = np.nonzero((bits(out[:, 3:]) != bits(ref.rows[:, 3:])).any(1))[0]
            assert len(bad) == 0, (ctx, "gather", dist, len(bad), bad[:4], out[bad[:2]], ref.rows[bad[:2]])
            assert st.rays == self.kw.get("samples", K) * self.valid and st.paths == len(self.rec), (ctx, "gather", dist, st.rays)
            if dist == 0.0:
                assert same(out, ref.rows), (ctx, "gather: the whole record", np.nonzero((bits(out) != bits(ref.rows)).any(1))[0][:4])
                if not lit:  # §12.1 (b) on the device's own two calls
                    one, st1 = call(P, r, self.rec, host=host, ray_eps=self.eps, max_depth=1, rr_start=0, **self.kw)
                    assert same(one, out) and st1.rays == ref.rays, (ctx, "(b)")
            outs.append(out)
        return outs


def on_layouts(P, r, refs, layouts, ctx, deep=False):
    """Lit and emitter-free scene committed on every layout of `layouts`: the checker's bits each time, and so the same on all."""
    first = None
    for width in layouts:
        outs = []
        for lit in (True, False):
            r.SetScene(refs.lit if lit else refs.dark, width)
            assert not deep or r.BvhInfo().stack_need > 12, (ctx, width, r.BvhInfo().stack_need)
            outs += refs.hold(P, r, ctx + (width, lit), lit=lit)
        first = first or outs
        assert all(same(a, b) for a, b in zip(outs, first)), (ctx, "layouts differ", width)
    return first


def alternating(P):
    return [w | (P.native.PT_BVH_BUILD_LBVH if i % 2 else 0) for i, w in enumerate(LAYOUTS)]


@pytest.mark.parametrize("name", ["layers", "duplicates", "soup", "spheres64"])
def test_adversarial_scenes(P, pto, renderer, name):
    """A1. Stacked layers (every ray's stack spills past the 12 LDS entries into the lane's overflow column: the probe set on the camera
    origin, tests/test_gather_space.py walks its rays), exact ties on t across leaves, the 4000-triangle soup and the full sphere list;
    the first hits from both sides (soup: and triangle centroids), on every layout with the builders alternating."""
    assert LBVH == P.native.PT_BVH_BUILD_LBVH
    sd, pts, nrm, eps = G.space_case(P, pto, name)
    assert len(pts) >= 64 and (name == "layers" or len(pts) >= 400)
    refs = Refs(pto, sd, pts, nrm, eps)
    outs = on_layouts(P, renderer, refs, alternating(P), (name,), deep=name == "layers")
    assert any(refs.paths[d].rays > K * len(pts) for d in DEPTHS) and 0 < refs.sky[0.0].visibility.sum() < len(pts)
    assert np.isfinite(np.concatenate(outs)).all()


@pytest.mark.parametrize("name", geometry_space.PATH_TRACE + ["translate_glass_2/map", "scale_glass_+40/map"])
def test_geometry_space(P, pto, renderer, name):
    """A2. The cases whose path trace tests/test_gpu_geometry_space.py holds, at the first hits of the case's camera and with its
    ray_eps, on BVH4Q from the host builder and BVH2 from the GPU builder; /map: under an environment map whose every texel has its own
    colour. The needle trees need more than the 12 LDS entries."""
    base, _, env = name.partition("/")
    case = geometry_space.cases()[base]
    sd, pts, nrm, eps = G.space_case(P, pto, base)
    assert len(pts) >= 27 and eps == np.float32(case.ray_eps)
    env = env_checker.distinct(8) if env else None
    for e in [eps] + ([G.tight_eps(sd)] if case.family == "translate" else []):
        refs = Refs(pto, sd, pts, nrm, e, env=env)
        on_layouts(P, renderer, refs, (68, 2 | LBVH), (name, e), deep=base == "needles_0.0001")
        if e != eps or case.family != "translate":
            assert refs.paths[DEPTHS[0]].rays > K * len(pts) or case.family == "flat", (name, e)


def test_refit(P, pto, renderer):
    """A3. The tessellated box moved by UpdateGeometry, fed from a device tensor, to the offset of 65537 and into needles: both gathers
    at the first hits of the moved scene equal the checker on the moved scene data; after updating back they are the outputs of before
    the update bit for bit."""
    import torch
    base, moved = geometry_space.refit_cases()
    moved = [c for c in moved if c.name in ("refit_translate_tess_2", "refit_needles")]
    assert len(moved) == 2
    home = Refs(pto, base, *G.first_hits(P, pto, base, step=2), G.EPS)
    there = []
    for case in moved:
        pts, nrm = G.first_hits(P, pto, case.sd, step=2)
        there.append((case, [Refs(pto, case.sd, pts, nrm, eps)
                             for eps in [case.ray_eps] + ([G.tight_eps(case.sd)] if case.family == "translate" else [])]))
    device = lambda v: torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda()
    for width in (68, 2 | LBVH):
        renderer.SetScene(home.lit, width)
        before = home.hold(P, renderer, ("home", width))
        for case, refs in there:
            renderer.UpdateGeometry(verts=device(case.sd.verts), spheres=case.sd.spheres)
            for ref in refs:
                ref.hold(P, renderer, (case.name, width, ref.eps), host=False)
            renderer.UpdateGeometry(verts=device(base.verts), spheres=base.spheres)
            after = home.hold(P, renderer, ("back from", case.name, width))
            assert all(same(a, b) for a, b in zip(after, before)), (case.name, width)


@pytest.mark.parametrize("scene,samples,n", [("glass", 64, GRID + 257), ("layers", 64, GRID + 257), ("glass", 16, 4 * GRID + 259),
                                             ("glass", 1, 64 * GRID + 65)])
def test_past_one_grid(P, pto, renderer, scene, samples, n):
    """A4. More points than one grid of 16384 one-wave workgroups holds (64, 4 and 1 points per wave at K = 1, 16 and 64): the waves
    take a second pass of the grid-stride loop, with their rows cleared, their samples restarted, their LDS and overflow columns
    (layers) used again and their counters carried over. Every index has its own key, so the point set is repeated cyclically. Three
    invalid points lie in the second pass.
    (i) the call equals the calls of at most one grid each with point_offset = the part's start, pt_stats::rays included, from host
    and from device memory; (ii) the checker on the first 64 points, the 64 across the grid's end and the last 321; and the invalid
    points give the sentinel rows and leave every other row what it is without them."""
    per_wave = 64 >> {1: 0, 16: 4, 64: 6}[samples]
    one = GRID * per_wave
    assert one < n < 2 * one and (samples != 16 or n % 4 != 0)
    sd, p0, n0, eps = G.space_case(P, pto, scene)
    pts, nrm = G.tiled(p0, n0, n)
    invalid = [n - 40, n - 5, n - 4]
    assert min(invalid) >= one
    tail = n - 321
    clean_rec = G.records(pts[tail:], nrm[tail:])
    pts[invalid[0], 1] = np.nan
    nrm[invalid[1], 0] = np.inf
    nrm[invalid[2]] = 0.0
    ok = np.ones(n, bool)
    ok[invalid] = False
    lit = dataclasses.replace(sd, sky=SKY)
    osc, dosc = pto.Scene(lit), pto.Scene(GP.without_emission(lit))
    osc.build_own_bvh()
    dosc.build_own_bvh()
    renderer.SetScene(lit, 68 if scene == "layers" else 2)
    assert scene != "layers" or renderer.BvhInfo().stack_need > 12
    rec = G.records(pts, nrm)
    runs = [(0, 64), (one - 32, one + 32), (tail, n)]
    for paths in (True, False):
        kw = dict(samples=samples, ray_eps=eps, paths=paths, max_depth=2)
        big, st = call(P, renderer, rec, **kw)
        dev, sd_ = call(P, renderer, rec, host=False, **kw)
        assert same(dev, big) and sd_.rays == st.rays, (paths, "host and device memory")
        parts = [call(P, renderer, rec[a:b], point_offset=a, **kw) for a, b in ((0, one), (one, n))]
        joined = np.concatenate([o for o, _ in parts])
        bad = np.nonzero((bits(big) != bits(joined)).any(1))[0]
        assert len(bad) == 0, (paths, "(i)", len(bad), bad[:4], big[bad[:2]], joined[bad[:2]])
        assert st.rays == sum(s.rays for _, s in parts) and st.paths == n, (paths, st.rays, st.paths)
        assert paths or st.rays == samples * (n - 3)
        for a, b in runs:
            ref = GP.gather(osc if paths else dosc, pts[a:b], nrm[a:b], samples=samples, ray_eps=eps, point_offset=a,
                            max_depth=2 if paths else 1, rr_start=3 if paths else 0)
            bad = np.nonzero((bits(big[a:b]) != bits(ref.rows)).any(1))[0]
            assert len(bad) == 0, (paths, "(ii)", a, b, len(bad), bad[:4], big[a + bad[:2]], ref.rows[bad[:2]])
        assert (big[~ok] == SENTINEL).all() and np.isfinite(big).all()
        clean, _ = call(P, renderer, clean_rec, point_offset=tail, **kw)
        assert same(clean[ok[tail:]], big[tail:][ok[tail:]]) and (clean[:, 3] >= 0).all(), (paths, "the invalid points' neighbours")


def test_key_sums_wrap(P, pto, renderer):
    """A5. §12: point_offset + i and sample_offset + k wrap around in u32. Eight points at K = 16 from point_offset 2^32 - 3 are three
    points from there and five from 0, and the checker's; 64 samples from sample_offset 2^32 - 16 are the checker's, and their visible
    count is that of the 16 samples up to 2^32 plus that of the 48 from 0."""
    sd, p0, n0, eps = G.space_case(P, pto, "glass")
    idx = np.arange(8) * 37
    pts, nrm = p0[idx], n0[idx]
    lit = dataclasses.replace(sd, sky=SKY)
    osc, dosc = pto.Scene(lit), pto.Scene(GP.without_emission(lit))
    renderer.SetScene(lit, 0)
    rec = G.records(pts, nrm)
    cnt = lambda o, k: np.rint(o[:, 3].astype(np.float64) * k).astype(np.int64)
    for paths in (True, False):
        ref = lambda **kw: GP.gather(osc if paths else dosc, pts, nrm, ray_eps=eps, max_depth=8 if paths else 1, rr_start=3 if paths else 0, **kw)
        kw = dict(ray_eps=eps, paths=paths)
        whole, st = call(P, renderer, rec, samples=16, point_offset=0xFFFFFFFD, **kw)
        a, sa = call(P, renderer, rec[:3], samples=16, point_offset=0xFFFFFFFD, **kw)
        b, sb = call(P, renderer, rec[3:], samples=16, point_offset=0, **kw)
        want = ref(samples=16, point_offset=0xFFFFFFFD)
        assert same(whole, np.concatenate([a, b])) and st.rays == sa.rays + sb.rays, paths
        assert same(whole, want.rows) and st.rays == want.rays, paths
        plain, _ = call(P, renderer, rec, samples=16, **kw)
        assert not same(plain, whole), paths
        wrapped, st = call(P, renderer, rec, sample_offset=0xFFFFFFF0, **kw)
        want = ref(sample_offset=0xFFFFFFF0)
        assert same(wrapped, want.rows) and st.rays == want.rays, paths
        lo, _ = call(P, renderer, rec, samples=16, sample_offset=0xFFFFFFF0, **kw)
        hi, _ = call(P, renderer, rec, samples=48, sample_offset=0, **kw)
        assert np.array_equal(cnt(lo, 16) + cnt(hi, 48), cnt(wrapped, K)) and 0 < cnt(wrapped, K).sum() < 8 * K, paths
