"""Experiment: pt_display (docs/SPEC.md §10) — what its three kernels cost; the table of DESIGN.md §13.

At 1920x1080 and 3840x2160, on a rendered frame of the 1M-triangle Cornell box (4 spp) and on a flat image (every pixel 0.18: all of
them in one histogram bin, the worst case for same-address atomics), put into the framebuffer through pt_assemble_tiles:
  metering  extend_ms of an AUTO call: the memset of the 512 words, k_display_histogram and k_display_resolve, between two events
  resolve   extend_ms of an AUTO call on a 1x1 frame: the same three with nothing to count — what the metering costs beyond its stream
  tone      other_ms: k_display_tone (ACES, sRGB encode)
each the median [min, max] of REPS warm calls from pt_stats after three warm-up calls, with the bytes the kernel must move (16 B read per
pixel for the histogram, 16 B read + 4 B written for the tone pass) over the median, beside the 6.29 TB/s a float4 copy sustains. Event
timing of kernels this short includes the gap between launches: read the numbers as call cost, not as a kernel's pure run time. (The
rejected histogram kernel — ballot aggregation per wave before the LDS atomics — was timed by this script, alternating with the kept
one in one process, before it was removed: DESIGN.md §13 has both columns.)
usage: python tools/exp_display.py [--reps 20] [--detail 1000000]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pathtracing_amd as P  # noqa: E402

N = P.native
SUSTAINED = 6.29e12  # B/s, float4 copy (README)


def mrange(xs):
    xs = sorted(xs)
    return np.median(xs), f"{np.median(xs) * 1e3:8.1f} us [{xs[0] * 1e3:.1f}, {xs[-1] * 1e3:.1f}]"


def assemble(r, img):
    """`img` ((h, w, 4) float32) into the framebuffer: tile-major, SPEC §6 slot order, spp = 1."""
    import torch
    h, w = img.shape[:2]
    p = P.make_params(w, h, spp=1, max_depth=1)
    lay = P.tile_layout(p)
    ts = lay.tile_size
    buf = np.zeros((lay.tiles_per_rank, ts // 8, ts // 8, 8, 8, 4), np.float32)
    y, x = np.mgrid[0:h, 0:w]
    buf[(y // ts) * lay.tiles_x + x // ts, (y % ts) // 8, (x % ts) // 8, y % 8, x % 8] = img
    g = torch.from_numpy(buf.reshape(-1)).cuda()
    torch.cuda.synchronize()
    r.Params = p
    r.AssembleTiles(g.data_ptr(), g.numel())
    torch.cuda.synchronize()


def timed(r, reps, **kw):
    """([extend_ms], [other_ms]) of `reps` calls after three warm-up calls."""
    out = ([], [])
    for k in range(reps + 3):
        st = r.Display(**kw)
        if k >= 3:
            out[0].append(st.extend_ms); out[1].append(st.other_ms)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--detail", type=int, default=1_000_000)
    a = ap.parse_args()
    r = P.Renderer(P.Window(1920, 1080))
    r.Init()
    try:
        assemble(r, np.full((1, 1, 4), 0.18, np.float32))
        res = timed(r, a.reps, curve="aces", auto=True, reset=True)
        floor_ms, text = mrange(res[0])
        print(f"resolve (1x1 frame: memset + empty histogram + resolve)   {text}")
        for w, h in ((1920, 1080), (3840, 2160)):
            n = w * h
            r.SetScene(P.make_scene(N.PT_SCENE_CORNELL_TESS, a.detail, 0x5EED0001, w, h), 0)
            for label in ("rendered", "flat"):
                if label == "rendered":
                    r.Params = P.make_params(w, h, spp=4, max_depth=8, streams=4)
                    r.Render(0.0)
                else:
                    assemble(r, np.full((h, w, 4), 0.18, np.float32))
                res = timed(r, a.reps, curve="aces", auto=True, reset=True)
                bins = int(np.count_nonzero(r.ReadDisplayHistogram()))
                print(f"== {w}x{h} {label}: {bins} bins in use, exposure {r.DisplayInfo().exposure:.4g}")
                med, text = mrange(res[0])
                hist_ms = max(med - floor_ms, 1e-6)
                print(f"  metering                  {text}   histogram alone ~{hist_ms * 1e3:6.1f} us = {16 * n / (hist_ms * 1e-3) / 1e12:5.2f} TB/s "
                      f"({16 * n / (hist_ms * 1e-3) / SUSTAINED:4.2f} of sustained)")
                med, text = mrange(res[1])
                print(f"  tone (ACES, sRGB)         {text}   {20 * n / (med * 1e-3) / 1e12:5.2f} TB/s ({20 * n / (med * 1e-3) / SUSTAINED:4.2f} of sustained)")
                med, text = mrange(timed(r, a.reps, curve="aces", linear=True)[1])
                print(f"  tone (ACES, LINEAR)       {text}   {20 * n / (med * 1e-3) / 1e12:5.2f} TB/s")
    finally:
        r.Dispose()


if __name__ == "__main__":
    main()
