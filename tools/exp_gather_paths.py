"""Experiment: pt_gather_paths (docs/SPEC.md §12.1) beside pt_render and pt_gather. GPU only.

Points: the first hits of a 1920x1080 frame (tools/exp_gather.py's) of plain Cornell (BVH2) and of the 1M-triangle tessellated Cornell box
(BVH4Q); K = 64 samples per point, max_depth 8, rr_start 3, ray_eps 1e-3, unbounded.
  leg A: pt_gather_paths on device records; pt_stats.gpu_ms and pt_stats.rays (the segments traced).
  leg B: a plain pt_render frame of the same scene at 64 spp, max_depth 8, 8 streams, on the one-ray-per-lane extend kernel (extend_kernel 1,
         one loop): the rate the same traversal and shading reach inside k_extend; pt_stats.gpu_ms and rays.
  leg C: pt_gather (occlusion rays only) on the same records.
Warm: 3 calls of each leg first, then REPS rounds with the legs alternating; median, best and spread (max - min) in ms, Grays/s at the median.
usage: python tools/exp_gather_paths.py [cornell,tess [repetitions]]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pathtracing_amd as P  # noqa: E402
from exp_gather import EPS, H, K, SEED, W, first_hit_points  # noqa: E402

N = P.native
REPS, DEPTH, RR = 11, 8, 3


def line(name, ms, rays):
    med = float(np.median(ms))
    return (f"  {name}: median {med:8.3f} ms   best {min(ms):8.3f} ms   spread {max(ms) - min(ms):7.3f} ms   {rays / 1e6:8.1f} Mrays   "
            f"{rays / med / 1e6:7.2f} Grays/s")


def main():
    which = sys.argv[1].split(",") if len(sys.argv) > 1 else ["cornell", "tess"]
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else REPS
    cfg = {"cornell": (N.PT_SCENE_CORNELL, 0), "tess": (N.PT_SCENE_CORNELL_TESS, 1 << 20)}
    r = P.Renderer(P.Window(W, H))
    r.Init()
    try:
        for name in which:
            sd = P.make_scene(*cfg[name], 0x5EED0001, W, H)
            r.SetScene(sd, 0)
            r.SetTuning(extend_kernel=1, loops=1)
            p, n = first_hit_points(r, sd.cam)
            dp, dn = torch.from_numpy(p).cuda(), torch.from_numpy(n).cuda()
            torch.cuda.synchronize()
            frame = P.make_params(W, H, spp=K, max_depth=DEPTH, rr_start=RR, streams=8)
            a_ms, b_ms, c_ms = [], [], []
            for rep in range(reps + 3):
                E, vis, bent, sa = r.GatherPaths(dp, dn, samples=K, seed=SEED, ray_eps=EPS, max_depth=DEPTH, rr_start=RR)
                r.Params = frame
                sb = r.Render(0.0)
                _, _, _, sc = r.Gather(dp, dn, samples=K, seed=SEED, ray_eps=EPS)
                if rep >= 3:
                    a_ms.append(sa.gpu_ms); b_ms.append(sb.gpu_ms); c_ms.append(sc.gpu_ms)
            print(f"{name}: layout {r.BvhInfo().width}, {len(p)} points x {K} samples, max_depth {DEPTH}; mean E {[round(float(x), 4) for x in E.mean(0)]}, "
                  f"mean visibility {float(vis.mean()):.4f}, segments per sample {sa.rays / (len(p) * K):.3f}; frame: kernel {int(sb.reserved[0])}, "
                  f"segments per sample {sb.rays / (W * H * K):.3f}")
            print(line("A pt_gather_paths          ", a_ms, sa.rays))
            print(line("B pt_render (one ray / lane)", b_ms, sb.rays))
            print(line("C pt_gather                ", c_ms, sc.rays), flush=True)
    finally:
        r.Dispose()


if __name__ == "__main__":
    main()
