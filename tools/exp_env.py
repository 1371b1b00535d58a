"""Experiment: environment-map lighting (pt_scene_set_environment, docs/SPEC.md §11) against the constant sky.

  cost  : ms per 1080p / 64 spp frame (best and mean of 20 warm frames) of the 1M-triangle soup (C3) and Cornell (C2): with a constant
          sky and no environment, on the kernel the scene's probe picks and on the forced one-ray-per-lane kernel; and with the sun-sky
          map at n = 64 and n = 1024, plain and with PT_FLAG_NEXT_EVENT. --sky-only runs the first part alone (it uses nothing the
          parent of this feature lacks, so the same script measures that commit).
  error : on the sun-lit soup at 480 x 270, RMSE of 64-spp frames against a converged frame (NEE, 8192 spp, another seed) and the GPU
          time each took; (mse_plain * ms_plain) / (mse_nee * ms_nee) is the time-to-equal-error ratio, as in tools/exp_nee.py.
Usage: python tools/exp_env.py [--sky-only] [--frames 20] [--out file.json]"""
import dataclasses
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pathtracing_amd as P  # noqa: E402

N = P.native
SCENES = {"C3 soup 1M": (N.PT_SCENE_TRIANGLE_SOUP, 1 << 20), "C2 cornell": (N.PT_SCENE_CORNELL, 0)}
SUN = ((0.35, 0.8, 0.5), (40.0, 36.0, 30.0), 0.95, (0.3, 0.4, 0.6))


def frames(r, w, h, spp, flags, count, **kw):
    r.Params = P.make_params(w, h, spp=spp, max_depth=8, streams=8, flags=flags, **kw)
    r.Render(0.0)  # warm (allocation, first touch, the scene's kernel probe)
    r.Render(0.0)
    st = [r.Render(0.0) for _ in range(count)]
    ms = [s.gpu_ms for s in st]
    return {"best_ms": float(min(ms)), "mean_ms": float(np.mean(ms)), "rays": int(st[-1].rays), "kernel": int(st[-1].reserved[0])}


def error(r, sd, w=480, h=270, spp=64, ref_spp=8192):
    r.SetScene(sd, 0)
    for k in range(ref_spp // 512):
        r.Params = P.make_params(w, h, spp=512, max_depth=8, streams=8, seed=77, sample_offset=512 * k,
                                 flags=N.PT_FLAG_NEXT_EVENT | (N.PT_FLAG_ACCUMULATE if k else 0))
        r.Render(0.0)
    ref = r.ReadFramebuffer()[..., :3].astype(np.float64)
    out = {}
    for nee in (False, True):
        res = frames(r, w, h, spp, N.PT_FLAG_NEXT_EVENT if nee else 0, 3)
        img = r.ReadFramebuffer()[..., :3].astype(np.float64)
        out["nee" if nee else "plain"] = {"ms": res["mean_ms"], "rmse": float(np.sqrt(np.mean((img - ref) ** 2)))}
    p, n = out["plain"], out["nee"]
    out["time_to_equal_error"] = (p["rmse"] ** 2 * p["ms"]) / (n["rmse"] ** 2 * n["ms"])
    out["rmse_ratio_equal_spp"] = p["rmse"] / n["rmse"]
    return out


def main():
    a = sys.argv
    out_path = a[a.index("--out") + 1] if "--out" in a else None
    count = int(a[a.index("--frames") + 1]) if "--frames" in a else 20
    sky_only = "--sky-only" in a
    r = P.Renderer(P.Window(1920, 1080))
    r.Init()
    res = {}
    try:
        for name, (kind, detail) in SCENES.items():
            sd = dataclasses.replace(P.make_scene(kind, detail, 0x5EED0001, 1920, 1080), sky=np.array([0.3, 0.4, 0.6], np.float32))
            r.SetScene(sd, 0)
            row = {"sky": frames(r, 1920, 1080, 64, 0, count), "sky one-ray-per-lane": frames(r, 1920, 1080, 64, N.PT_FLAG_EXTEND_SIMPLE, count),
                   "sky one-ray-per-lane nee": frames(r, 1920, 1080, 64, N.PT_FLAG_EXTEND_SIMPLE | N.PT_FLAG_NEXT_EVENT, count)}
            if not sky_only:
                for n in (64, 1024):
                    r.SetEnvironment(P.sun_sky_environment(n, *SUN))
                    for nee in (False, True):
                        row[f"env n={n} {'nee' if nee else 'plain'}"] = frames(r, 1920, 1080, 64, N.PT_FLAG_NEXT_EVENT if nee else 0, count)
            res[name] = row
            print(name, json.dumps(row), flush=True)
        if not sky_only:
            sd = dataclasses.replace(P.make_scene(N.PT_SCENE_TRIANGLE_SOUP, 1 << 20, 0x5EED0001, 480, 270), sky=np.zeros(3, np.float32),
                                     environment=P.sun_sky_environment(64, *SUN))
            res["error soup 1M"] = error(r, sd)
            print("error soup 1M", json.dumps(res["error soup 1M"]), flush=True)
    finally:
        r.Dispose()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
