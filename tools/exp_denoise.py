"""Experiment: pt_denoise (docs/SPEC.md §8) — what it costs and what it buys. GPU only; the tables of DESIGN.md §10.

(1) Cost at 1920x1080: the guide pass (pt_stats.extend_ms) and the filter (other_ms) for 1..5 passes, on C2 (Cornell) and on the
    1M-triangle headline scene; median [min, max] of REPS calls after two warm-up calls, next to the 64-spp frame itself.
(2) Quality at 1920x1080 against a converged device frame (16384 spp; the device equals the oracle bit for bit): RMSE of the noisy and
    the denoised frame at 1, 4 and 16 spp, C1 with and without NEE and C4; linear radiance and displayed (clamped to [0, 1], what the
    8-bit image shows); the plain B3 blur (PT_DENOISE_NO_EDGE_STOPS) as the control.
(3) Equal GPU time: the denoised 4-spp frame (frame + denoise gpu_ms) against a plain frame of as many samples as that time buys.
(4) The sigma sweep around the defaults on the 4-spp frames of (2) (geometric mean over C1+NEE and C4 of denoised / noisy displayed RMSE).
usage: python tools/exp_denoise.py [--reps 7] [--only cost|quality|sweep]"""
import argparse
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pathtracing_amd as P  # noqa: E402

N = P.native
W, H = 1920, 1080
REF_SPP = 16384


def mrange(xs):
    xs = sorted(xs)
    return f"{np.median(xs):7.3f} [{xs[0]:.3f}, {xs[-1]:.3f}]"


def rmse(a, ref, display):
    a, ref = a[..., :3].astype(np.float64), ref[..., :3].astype(np.float64)
    if display:
        a, ref = np.clip(a, 0, 1), np.clip(ref, 0, 1)
    return float(np.sqrt(np.mean((a - ref) ** 2)))


def frame(r, spp, flags, seed, streams=8):
    r.Params = P.make_params(W, H, spp=spp, max_depth=8, streams=min(streams, spp), seed=seed, flags=flags)
    st = r.Render(0.0)
    return r.ReadFramebuffer(), st


def cost(r, reps):
    print("== cost at 1920x1080 (ms: median [min, max])")
    for label, kind, detail in (("C2 cornell", N.PT_SCENE_CORNELL, 0), ("headline 1M tris", N.PT_SCENE_CORNELL_TESS, 1_000_000)):
        r.SetScene(P.make_scene(kind, detail, 0x5EED0001, W, H), 0)
        fr = []
        for k in range(reps + 1):
            _, st = frame(r, 64, 0, 0x5EED0001)
            if k:
                fr.append(st.gpu_ms)
        print(f"{label:18s} frame 64 spp        gpu_ms {mrange(fr)}")
        for it in (1, 2, 3, 4, 5):
            g, f, t = [], [], []
            for k in range(reps + 2):
                st = r.Denoise(iterations=it)
                if k >= 2:
                    g.append(st.extend_ms); f.append(st.other_ms); t.append(st.gpu_ms)
            print(f"{label:18s} {it} passes  guides {mrange(g)}  filter {mrange(f)}  total {mrange(t)}")


def quality(r, sweep_only=False):
    cases = {}
    for label, kind, flags in (("C1 NEE", N.PT_SCENE_CORNELL, N.PT_FLAG_NEXT_EVENT), ("C1", N.PT_SCENE_CORNELL, 0),
                               ("C4", N.PT_SCENE_CORNELL_GLASS, 0)):
        if sweep_only and label == "C1":
            continue
        r.SetScene(P.make_scene(kind, 0, 3, W, H), 0)
        ref, _ = frame(r, REF_SPP, flags, 99)
        cases[label] = (kind, flags, ref)
        if sweep_only:
            continue
        print(f"== quality {label} (RMSE against {REF_SPP} spp; linear | displayed)")
        for spp in (1, 4, 16):
            noisy, st = frame(r, spp, flags, 7)
            d = r.Denoise()
            den = r.ReadDenoised()
            r.Denoise(edge_stops=False)
            blur = r.ReadDenoised()
            print(f"  {spp:2d} spp  noisy {rmse(noisy, ref, 0):.4f} | {rmse(noisy, ref, 1):.4f}   denoised {rmse(den, ref, 0):.4f} | "
                  f"{rmse(den, ref, 1):.4f}   blur {rmse(blur, ref, 0):.4f} | {rmse(blur, ref, 1):.4f}   frame {st.gpu_ms:.2f} ms + denoise {d.gpu_ms:.2f} ms")
            if spp == 4:  # equal time: how many plain samples the denoised frame's time buys
                _, one = frame(r, 64, flags, 11)
                n = max(1, int(round((st.gpu_ms + d.gpu_ms) / (one.gpu_ms / 64))))
                plain, pst = frame(r, n, flags, 13)
                print(f"  equal time: denoised 4 spp ({st.gpu_ms + d.gpu_ms:.2f} ms) {rmse(den, ref, 0):.4f} | {rmse(den, ref, 1):.4f}   "
                      f"plain {n} spp ({pst.gpu_ms:.2f} ms) {rmse(plain, ref, 0):.4f} | {rmse(plain, ref, 1):.4f}")
    return cases


def sweep(r, cases):
    print("== sigma sweep, 4 spp (geometric mean of denoised / noisy displayed RMSE over C1 NEE and C4; linear in brackets)")
    frames = {}
    for label in ("C1 NEE", "C4"):
        kind, flags, ref = cases[label]
        frames[label] = (kind, flags, ref)
    res = []
    grid = list(itertools.product((2, 3, 4, 5), (4.0, 16.0, 64.0), (0.0625, 0.25), (0.0078125, 0.015625, 0.0625), (0.25,)))
    for label, (kind, flags, ref) in frames.items():
        r.SetScene(P.make_scene(kind, 0, 3, W, H), 0)
        noisy, _ = frame(r, 4, flags, 7)
        en, el = rmse(noisy, ref, 1), rmse(noisy, ref, 0)
        for i, (it, sc, sn, sz, sa) in enumerate(grid):
            r.Denoise(iterations=it, sigma_color=sc, sigma_normal=sn, sigma_depth=sz, sigma_albedo=sa)
            den = r.ReadDenoised()
            if len(res) <= i:
                res.append([(it, sc, sn, sz, sa), [], []])
            res[i][1].append(rmse(den, ref, 1) / en); res[i][2].append(rmse(den, ref, 0) / el)
    res.sort(key=lambda x: np.exp(np.mean(np.log(x[1]))))
    for prm, disp, lin in res[:12]:
        print(f"  passes {prm[0]} sigma_c {prm[1]:6g} sigma_n {prm[2]:6g} sigma_z {prm[3]:9g} sigma_a {prm[4]:5g}   "
              f"{np.exp(np.mean(np.log(disp))):.3f} {np.round(disp, 3).tolist()} ({np.round(lin, 3).tolist()})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", choices=["cost", "quality", "sweep"])
    a = ap.parse_args()
    r = P.Renderer(P.Window(W, H))
    r.Init()
    try:
        if a.only in (None, "cost"):
            cost(r, a.reps)
        if a.only in (None, "quality", "sweep"):
            cases = quality(r, sweep_only=a.only == "sweep")
            if a.only in (None, "sweep"):
                sweep(r, cases)
    finally:
        r.Dispose()


if __name__ == "__main__":
    main()
