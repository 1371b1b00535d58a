"""Experiment: pt_denoise_temporal (docs/SPEC.md §9) — what it costs and what it buys; the tables of DESIGN.md §12.

(1) cpu: the quality experiment on the oracle's frames with the scalar checkers (no GPU): C1 and C4 at 96x72, 8 frames of 1 spp (and C1 at
    4 spp) along the camera path of tests/temporal_cases.py, the default §8.2 filter over the last frame alone and over the accumulated
    image, RMSE against a 2048-spp oracle frame at the last camera; then the sweep of tau_p and tau_n on the same sequences.
(2) cost at 1920x1080 on C2: shade_ms of the temporal pass for a still and for a moving camera, beside one à-trous pass of the same call
    (other_ms of a one-pass filter) and the guide pass; median [min, max] of REPS calls after two warm-up calls.
(3) quality on the device: the experiment of (1) at 320x240 against a 4096-spp device frame.
usage: python tools/exp_temporal.py [--reps 7] [--only cpu|cost|quality]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, d)
import pathtracing_amd as P  # noqa: E402
import temporal_cases as tc  # noqa: E402  (test infrastructure: the camera path and the error measures the tests use)

N = P.native
W, H = 1920, 1080


def mrange(xs):
    xs = sorted(xs)
    return f"{np.median(xs):7.4f} [{xs[0]:.4f}, {xs[-1]:.4f}]"


def cpu():
    import denoise_checker as dc
    import pto
    import temporal_checker as tr
    w, h, frames = 96, 72, 8
    print(f"== checker, {w}x{h}, {frames} frames, RMSE against 2048 spp (filter alone -> temporal + filter)")
    seqs = {}
    for label, kind, spp in (("C1 1 spp", N.PT_SCENE_CORNELL, 1), ("C4 1 spp", N.PT_SCENE_CORNELL_GLASS, 1), ("C1 4 spp", N.PT_SCENE_CORNELL, 4)):
        sd = P.make_scene(kind, 0, 3, w, h)
        cams = tc.camera_path(sd.cam, frames)
        seq = []
        for k, cam in enumerate(cams):
            scene = pto.Scene(tc.with_camera(sd, cam))
            seq.append((pto.render(scene, P.make_params(w, h, spp=spp, max_depth=8, seed=1000 + k, streams=spp))[0], dc.guides(pto, scene, w, h), cam))
        ref = pto.render(scene, P.make_params(w, h, spp=2048, max_depth=8, seed=99, streams=8))[0]
        seqs[label] = (seq, ref)

    def run(label, p=None):
        seq, ref = seqs[label]
        hist, took = None, []
        for frame, g, cam in seq:
            res = tr.accumulate(frame, g, cam, hist, p)
            hist = res.history
            hits = g[..., 7].view(np.uint32) != tr.MISS
            took.append((res.length > 1)[hits].mean())
        alone, both = dc.filter(frame, g), dc.filter(res.image, g)
        return (tc.display_rmse(alone, ref), tc.display_rmse(both, ref)), (tc.linear_rmse(alone, ref), tc.linear_rmse(both, ref)), took[1:]

    for label in seqs:
        d, l, took = run(label)
        print(f"  {label}: displayed {d[0]:.4f} -> {d[1]:.4f} (ratio {d[1] / d[0]:.3f})   linear {l[0]:.4f} -> {l[1]:.4f}   "
              f"hit pixels with history, frames 2..{frames}: {min(took):.3f} .. {max(took):.3f}")
    print("== sweep of tau_p, tau_n (displayed ratio temporal + filter / filter alone: C1 1 spp, C4 1 spp, geometric mean; least history C1)")
    for tau_p in (2.0 ** -9, 2.0 ** -8, 2.0 ** -7, 2.0 ** -6, 2.0 ** -5):
        for tau_n in (0.5, 0.75, 0.875, 0.96875):
            rs, tk = [], []
            for label in ("C1 1 spp", "C4 1 spp"):
                d, _, took = run(label, tr.params(0, tau_p, tau_n))
                rs.append(d[1] / d[0]); tk.append(min(took))
            print(f"  tau_p 2^{int(np.log2(tau_p)):3d} tau_n {tau_n:7.5f}   {rs[0]:.3f} {rs[1]:.3f}  {np.sqrt(rs[0] * rs[1]):.3f}   {tk[0]:.3f}")


def cost(r, reps):
    print("== cost at 1920x1080, C2 (ms: median [min, max])")
    sd = P.make_scene(N.PT_SCENE_CORNELL, 0, 0x5EED0001, W, H)
    r.SetScene(sd, 0)
    cams = tc.camera_path(sd.cam, reps + 3)
    for label, moving in (("still camera", False), ("moving camera", True)):
        g, t, f, paths = [], [], [], []
        for k in range(reps + 2):
            r.SetCamera(cams[k + 1] if moving else cams[0])
            r.Params = P.make_params(W, H, spp=1, max_depth=8, seed=1000 + k)
            r.Render(0.0)
            st = r.DenoiseTemporal(iterations=1)
            if k >= 2:
                g.append(st.extend_ms); t.append(st.shade_ms); f.append(st.other_ms); paths.append(st.paths / float(W * H))
        print(f"  {label:14s} guides {mrange(g)}  temporal {mrange(t)}  one a-trous pass {mrange(f)}  pixels with history {np.mean(paths):.3f}")


def quality(r):
    print("== quality on the device, 320x240, 8 frames of 1 spp, RMSE against 4096 spp (filter alone -> temporal + filter)")
    for label, kind in (("C1", N.PT_SCENE_CORNELL), ("C4", N.PT_SCENE_CORNELL_GLASS)):
        q = tc.device_quality(P, r, kind, 320, 240)
        d, l = q["display"], q["linear"]
        print(f"  {label}: displayed {d[0]:.4f} -> {d[1]:.4f} (ratio {d[1] / d[0]:.3f})   linear {l[0]:.4f} -> {l[1]:.4f}   "
              f"pixels with history in the last call {q['took']:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", choices=["cpu", "cost", "quality"])
    a = ap.parse_args()
    if a.only in (None, "cpu"):
        cpu()
    if a.only == "cpu":
        return
    r = P.Renderer(P.Window(W, H))
    r.Init()
    try:
        if a.only in (None, "cost"):
            cost(r, a.reps)
        if a.only in (None, "quality"):
            quality(r)
    finally:
        r.Dispose()


if __name__ == "__main__":
    main()
