"""-m gpu: the thin lens (pt_scene_set_lens, docs/SPEC.md §3.1) on the device across the lens and camera space (tests/lens_space.py has
the cases; tests/test_lens_space.py holds the checker to float64 on them without a device).

* Every (lens, camera) of the cross on three scenes: the frame is the checker's bit for bit, rays and paths too, or pt_render refuses
  the lens exactly where the checker does. The tessellated box in layouts 2 and 68 and from both builders; Cornell with
  PT_FLAG_NEXT_EVENT under two cameras.
* Every sample's closest hit, as ids of max_depth = 1 frames, against the float64 caster on lens64's rays, by the function that judged
  the checker.
* A refused lens changes nothing the context holds, and the next frame is the checker's; a radius of 0 is the pinhole whatever F is;
  ray queries, gathers and the guides do not see the lens."""
import numpy as np
import pytest

import camera_space as cs
import lens_checker as lc
import lens_device as ld
import lens_space as ls
from gather_device import same

pytestmark = pytest.mark.gpu

W, H = ls.W, ls.H
CROSS = ls.cross()
PAIR_IDS = [f"{lens}-{cam}" for lens, cam in CROSS]
LBVH = 0x100


def params(P, nee=False):
    return P.make_params(W, H, spp=4, streams=2, max_depth=4, flags=P.native.PT_FLAG_NEXT_EVENT if nee else 0)


def refused(P, r, ctx):
    """pt_render refuses the scene's lens: PT_ERR_INVALID_ARGUMENT, and the message names the lens."""
    with pytest.raises(P.PtException, match="lens") as e:
        r.Render(0.0)
    assert e.value.status == P.native.PT_ERR_INVALID_ARGUMENT, (ctx, str(e.value))


@pytest.mark.parametrize("lens,cam", CROSS, ids=PAIR_IDS)
def test_frames_across_the_cross(P, pto, renderer, lens, cam):
    """lens_device.check (frame, rays, paths, reserved[0] == 1, reserved[3] == 0, finite) at 4 spp, 2 streams, max_depth 4."""
    lens_v = ls.LENS_CASES[lens]
    for name in ls.SCENES:
        sd = ls.table(P, name)[cam]
        inside = lc.in_domain(pto, sd.cam, lens_v, W, H)
        for layout in ((2, 68, 68 | LBVH) if name == "box" else (ls.scene(P, name)[1],)):
            renderer.SetScene(sd, layout)
            renderer.SetLens(*lens_v)
            renderer.Params = params(P)
            if inside:
                ld.check(P, pto, renderer, (cam, name), sd, lens_v, renderer.Params, (lens, cam, name, layout))
            else:
                refused(P, renderer, (lens, cam, name, layout))


@pytest.mark.parametrize("cam", ["skewed", "far"])
def test_cornell_with_next_event(P, pto, renderer, cam):
    sd = cs.cases(P, cs.scene(P, "cornell")[0])[cam]
    lens_v = ls.LENS_CASES[ls.MODERATE]
    renderer.SetScene(sd, 0)
    renderer.SetLens(*lens_v)
    renderer.Params = params(P, nee=True)
    st = ld.check(P, pto, renderer, (cam, "cornell"), sd, lens_v, renderer.Params, (cam, "cornell", "nee"))
    assert st.rays > st.paths  # shadow rays were traced


@pytest.fixture(scope="module")
def refs(P, pto):
    triples = [(lens, cam, name) for lens, cam in CROSS for name in ls.scenes_of(P, lens, cam)
               if lc.in_domain(pto, ls.table(P, name)[cam].cam, ls.LENS_CASES[lens], W, H)]
    return ls.references(P, pto, triples)


@pytest.mark.parametrize("lens,cam", CROSS, ids=PAIR_IDS)
def test_device_hits_against_the_caster(P, pto, renderer, refs, lens, cam):
    """The id frames of lens_space.frame_ids from pt_render against the float64 caster on lens64's rays: no wrong sample, at most 1 %
    undecidable (lens_space.judge, which reads the reference alone) — and the ids are the checker's, so both leave out the same samples."""
    for name in ls.scenes_of(P, lens, cam):
        if (lens, cam, name) not in refs:
            continue  # refused: test_frames_across_the_cross
        ref = refs[(lens, cam, name)]
        renderer.SetScene(ref.sd, ls.scene(P, name)[1])
        renderer.SetLens(*ref.lens)

        def render(p):
            renderer.Params = p
            renderer.Render(0.0)
            return renderer.ReadFramebuffer()

        got = ls.frame_ids(render, P)
        share = ls.check(ref, got, (lens, cam, name))
        osc = pto.Scene(ref.sd)
        assert np.array_equal(got, ls.frame_ids(lambda p: lc.render(pto, osc, p, lens=ref.lens)[0], P)), (lens, cam, name)
        print(f"device hits {lens} under {cam} on {name}: undecidable {100 * share:.3f} %")


def out_of_domain(P):
    """[(lens values, camera)] under which a frame of `triangle` is refused: OUT_OF_DOMAIN under `default`, far_focus under SCALED."""
    t = ls.table(P, "triangle")
    return [(ls.LENS_CASES[n], t["default"].cam) for n in ls.OUT_OF_DOMAIN] + [(ls.LENS_CASES["far_focus"], t[ls.SCALED].cam)]


def test_refusals_change_nothing(P, pto):
    """On a context of its own: a frame through the moderate lens, denoised, accumulated over time and displayed; then every out-of-domain
    case is refused with PT_ERR_INVALID_ARGUMENT and a message that names the lens, and the framebuffer, the denoised, temporal and
    displayed images, the guides and the history compare equal before and after; the PT_FLAG_ACCUMULATE frame that follows is the one
    of the sequence without the refusals; and the next frame is the checker's."""
    N = P.native
    sd = ls.table(P, "triangle")["default"]
    lens_v = ls.LENS_CASES[ls.MODERATE]

    def sequence(with_refusals):
        r = P.Renderer(P.Window(W, H))
        r.Init()
        try:
            r.SetScene(sd, 0)
            r.SetLens(*lens_v)
            r.Params = P.make_params(W, H, spp=2, max_depth=4, streams=2)
            r.Render(0.0)
            r.Denoise()
            r.DenoiseTemporal()
            r.Display()
            kept = lambda: (r.ReadFramebuffer(), r.ReadDenoised(), r.ReadDisplay().astype(np.float32), r.ReadTemporal(), r.ReadGuides(),  # noqa: E731
                            r.ReadHistoryLength())
            before = kept()
            if with_refusals:
                for bad, cam in out_of_domain(P):
                    r.SetCamera(cam)
                    r.SetLens(*bad)
                    refused(P, r, (bad, "refusal"))
                    changed = [j for j, (a, b) in enumerate(zip(kept(), before)) if not same(np.asarray(a, np.float32), np.asarray(b, np.float32))]
                    assert not changed, (bad, "changed (0 framebuffer, 1 denoised, 2 display, 3 temporal, 4 guides, 5 history length)", changed)
                r.SetCamera(sd.cam)
                r.SetLens(*lens_v)
            r.Params = P.make_params(W, H, spp=2, max_depth=4, streams=2, sample_offset=2, flags=N.PT_FLAG_ACCUMULATE)
            st = r.Render(0.0)
            acc = r.ReadFramebuffer(), int(st.rays)
            r.Params = params(P)
            ld.check(P, pto, r, ("default", "triangle"), sd, lens_v, r.Params, "after the refusals")
            return acc
        finally:
            r.Dispose()

    a, b = sequence(True), sequence(False)
    assert same(a[0], b[0]) and a[1] == b[1], ("the accumulated frame differs", a[1], b[1])


def test_radius_zero_is_the_pinhole_whatever_f(P, pto, renderer):
    sd = ls.table(P, "triangle")["default"]
    renderer.SetScene(sd, 0)
    renderer.Params = params(P)
    st = renderer.Render(0.0)
    want = renderer.ReadFramebuffer(), (st.rays, st.paths, st.reserved[3])
    assert want[1][2] != 0  # the pinhole frame resolves sky pixels: a lens frame would not
    for (R, F), cam in out_of_domain(P):
        if R >= 1.0:
            continue  # the aperture's case: its F is inside the domain at any other radius
        renderer.SetCamera(cam)
        renderer.SetLens(ls.LENS_CASES[ls.MODERATE][0], F)
        refused(P, renderer, (F, "with a radius"))
        renderer.SetCamera(sd.cam)
        renderer.SetLens(0.0, F)
        st = renderer.Render(0.0)
        assert same(renderer.ReadFramebuffer(), want[0]) and (st.rays, st.paths, st.reserved[3]) == want[1], F


def test_queries_gathers_and_guides_ignore_an_out_of_domain_lens(P, pto, renderer):
    sd = ls.table(P, "box")["default"]
    renderer.SetScene(sd, 0)
    renderer.Params = params(P)
    renderer.Render(0.0)
    rng = np.random.default_rng(3)
    o = rng.uniform(-0.5, 0.5, (256, 3)).astype(np.float32)
    d = rng.normal(size=(256, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)

    def everything():
        renderer.Denoise(iterations=1)
        hits = renderer.TraceRays((o, d))[0]
        E, vis, bent, _ = renderer.Gather(o, d, samples=16, seed=7)
        return [np.ascontiguousarray(a).view(np.uint32).copy() for a in (renderer.ReadGuides(), renderer.ReadDenoised(), hits, E, vis, bent)]

    want = everything()
    for bad, cam in out_of_domain(P)[:4]:
        renderer.SetLens(*bad)
        for a, b in zip(want, everything()):
            assert np.array_equal(a, b), bad
    refused(P, renderer, "the lens was there")
