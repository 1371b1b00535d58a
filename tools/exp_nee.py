"""Experiment: next-event estimation (PT_FLAG_NEXT_EVENT, docs/SPEC.md §7) against the plain path tracer.

  speed : ms per 1080p / 64 spp frame, Grays/s and the shadow-ray share, with and without NEE, on C2 (Cornell), C4 (Cornell + glass +
          metal) and the 1M-triangle Cornell (median of 5 warm frames each)
  error : RMSE against a converged frame (NEE, 8192 spp, another seed) of 64-spp frames at 480 x 270, and the GPU time each took.
          For unbiased estimators MSE * time is constant, so the time the plain tracer needs to reach NEE's error is
          (mse_plain * ms_plain) / (mse_nee * ms_nee) times NEE's: the time-to-equal-error ratio.
Usage: python tools/exp_nee.py [--out file.json]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pathtracing_amd as P  # noqa: E402

N = P.native
SCENES = {"C2 cornell": (N.PT_SCENE_CORNELL, 0, 8), "C4 glass+metal": (N.PT_SCENE_CORNELL_GLASS, 0, 16),
          "1M-triangle cornell": (N.PT_SCENE_CORNELL_TESS, 1 << 20, 8)}


def frame(r, w, h, spp, depth, nee, seed=0x5EED0001, offset=0, acc=False):
    flags = (N.PT_FLAG_NEXT_EVENT if nee else 0) | (N.PT_FLAG_ACCUMULATE if acc else 0)
    r.Params = P.make_params(w, h, spp=spp, max_depth=depth, streams=8, seed=seed, flags=flags, sample_offset=offset)
    return r.Render(0.0)


def speed(r, depth):
    out = {}
    for nee in (False, True):
        frame(r, 1920, 1080, 64, depth, nee)  # warm (allocation, first touch)
        st = [frame(r, 1920, 1080, 64, depth, nee) for _ in range(5)]
        ms = float(np.median([s.gpu_ms for s in st]))
        out["nee" if nee else "plain"] = {"ms": ms, "rays": int(st[0].rays), "grays_s": st[0].rays / ms / 1e6}
    out["shadow_share"] = 1.0 - out["plain"]["rays"] / out["nee"]["rays"]
    out["ms_ratio"] = out["nee"]["ms"] / out["plain"]["ms"]
    return out


def error(r, depth, w=480, h=270, spp=64, ref_spp=8192):
    for k in range(ref_spp // 512):  # the converged frame: NEE, another seed, progressive
        frame(r, w, h, 512, depth, True, seed=77, offset=512 * k, acc=k > 0)
    ref = r.ReadFramebuffer()[..., :3].astype(np.float64)
    out = {}
    for nee in (False, True):
        frame(r, w, h, spp, depth, nee)
        st = [frame(r, w, h, spp, depth, nee) for _ in range(3)]
        img = r.ReadFramebuffer()[..., :3].astype(np.float64)
        out["nee" if nee else "plain"] = {"ms": float(np.median([s.gpu_ms for s in st])), "rmse": float(np.sqrt(np.mean((img - ref) ** 2)))}
    p, n = out["plain"], out["nee"]
    out["time_to_equal_error"] = (p["rmse"] ** 2 * p["ms"]) / (n["rmse"] ** 2 * n["ms"])
    out["rmse_ratio_equal_spp"] = p["rmse"] / n["rmse"]
    return out


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    r = P.Renderer(P.Window(1920, 1080))
    r.Init()
    res = {}
    try:
        for name, (kind, detail, depth) in SCENES.items():
            r.SetScene(P.make_scene(kind, detail, 0x5EED0001, 1920, 1080), 0)
            res[name] = {"speed": speed(r, depth)}
            r.SetScene(P.make_scene(kind, detail, 0x5EED0001, 480, 270), 0)
            res[name]["error"] = error(r, depth)
            print(name, json.dumps(res[name]), flush=True)
    finally:
        r.Dispose()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
