"""Experiment: pt_gather_paths with and without PT_GATHER_PATHS_NEXT_EVENT (docs/SPEC.md §12.2). GPU only.

Points: the first hits of a 1920x1080 frame (tools/exp_gather.py's) of plain Cornell (BVH2) and of the 1M-triangle tessellated Cornell box
(BVH4Q); K = 64 samples per point, max_depth 8, rr_start 3, ray_eps 1e-3, unbounded. Both calls run in one process on device records.
  time    : 3 warm rounds, then REPS rounds with the two calls alternating; pt_stats.gpu_ms: median, best and spread (max - min), and
            pt_stats.rays (plain: the segments; flagged: segments + shadow rays).
  variance: SEEDS bakes of each with seeds SEED .. SEED + SEEDS - 1; per point the unbiased variance of E over the seeds, summed over the
            channels, then the mean over the points (the variance of a texel of a K-sample bake).
  efficiency ratio = (var_plain * ms_plain) / (var_nee * ms_nee): above 1 the flag buys more than it costs.
usage: python tools/exp_gather_nee.py [cornell,tess [repetitions [seeds]]]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pathtracing_amd as P  # noqa: E402
from exp_gather import EPS, H, K, SEED, W, first_hit_points  # noqa: E402

N = P.native
REPS, SEEDS, DEPTH, RR = 11, 16, 8, 3


def line(name, ms, rays):
    med = float(np.median(ms))
    return (f"  {name}: median {med:8.3f} ms   best {min(ms):8.3f} ms   spread {max(ms) - min(ms):7.3f} ms   {rays / 1e6:8.1f} Mrays   "
            f"{rays / med / 1e6:7.2f} Grays/s")


def main():
    which = sys.argv[1].split(",") if len(sys.argv) > 1 else ["cornell", "tess"]
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else REPS
    seeds = int(sys.argv[3]) if len(sys.argv) > 3 else SEEDS
    cfg = {"cornell": (N.PT_SCENE_CORNELL, 0), "tess": (N.PT_SCENE_CORNELL_TESS, 1 << 20)}
    r = P.Renderer(P.Window(W, H))
    r.Init()
    try:
        for name in which:
            sd = P.make_scene(*cfg[name], 0x5EED0001, W, H)
            r.SetScene(sd, 0)
            p, n = first_hit_points(r, sd.cam)
            dp, dn = torch.from_numpy(p).cuda(), torch.from_numpy(n).cuda()
            torch.cuda.synchronize()
            bake = lambda flag, seed: r.GatherPaths(dp, dn, samples=K, seed=seed, ray_eps=EPS, max_depth=DEPTH, rr_start=RR, next_event=flag)
            ms = {False: [], True: []}
            for rep in range(reps + 3):
                for flag in (False, True):
                    E, vis, _, st = bake(flag, SEED)
                    if rep >= 3:
                        ms[flag].append(st.gpu_ms)
                    if rep == 0:
                        print(f"{name} {'flagged' if flag else 'plain  '}: mean E {[round(float(x), 4) for x in E.mean(0)]}, mean visibility "
                              f"{float(vis.mean()):.4f}, rays per sample {st.rays / (len(p) * K):.3f}")
            rays = {flag: bake(flag, SEED)[3].rays for flag in (False, True)}
            var = {}
            for flag in (False, True):
                s1 = torch.zeros((len(p), 3), dtype=torch.float64, device="cuda")
                s2 = torch.zeros_like(s1)
                for j in range(seeds):
                    E = bake(flag, SEED + j)[0].double()
                    s1 += E
                    s2 += E * E
                var[flag] = float(((s2 - s1 * s1 / seeds) / (seeds - 1)).sum(1).mean())
            mp, mn = float(np.median(ms[False])), float(np.median(ms[True]))
            print(f"{name}: layout {r.BvhInfo().width}, {len(p)} points x {K} samples, max_depth {DEPTH}, rr_start {RR}, {reps} rounds, {seeds} seeds")
            print(line("plain   pt_gather_paths", ms[False], rays[False]))
            print(line("flagged pt_gather_paths", ms[True], rays[True]))
            print(f"  shadow rays {(rays[True] - rays[False]) / 1e6:.1f} M; mean per-point variance of E: plain {var[False]:.6g}, flagged {var[True]:.6g} "
                  f"(ratio {var[False] / var[True]:.2f}); time ratio {mn / mp:.3f}; efficiency ratio {(var[False] * mp) / (var[True] * mn):.2f}", flush=True)
    finally:
        r.Dispose()


if __name__ == "__main__":
    main()
