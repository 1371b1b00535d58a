"""Experiment: sphere lights in next-event estimation (PT_FLAG_NEXT_EVENT_SPHERES / PT_GATHER_PATHS_SPHERE_LIGHTS, docs/SPEC.md §7.1) against
the plain path tracer and against next-event estimation without them. GPU only.

Scenes: Cornell (BVH2) and the 1M-triangle Cornell (BVH4Q) with the ceiling quad replaced by a lamp: an emissive sphere of radius 0.05.
  frames  : ms per 1080p / 64 spp / 8 streams frame (median of 5 warm frames), Grays/s and the shadow-ray share for plain, unflagged NEE
            (which finds the lamp by hits only) and flagged frames; RMSE of 480 x 270, 64-spp frames against a converged flagged frame of
            another seed, and the time-to-equal-error ratio (mse * ms) / (mse * ms)_flagged of each.
  gathers : the first hits of the 1080p frame (tools/exp_gather.py's, 1.08 M points on Cornell) x 64 paths: pt_stats.gpu_ms and rays,
            unflagged NEE and flagged alternating (median of 5), and the variance of E per point over 8 seeds, mean over the points.
Usage: python tools/exp_sphere_lights.py [--out file.json] [cornell,tess]"""
import dataclasses
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pathtracing_amd as P  # noqa: E402

N = P.native
SCENES = {"cornell": (N.PT_SCENE_CORNELL, 0), "tess": (N.PT_SCENE_CORNELL_TESS, 1 << 20)}
LAMP, EMISSION = (0.0, 0.6, 0.0, 0.05), (400.0, 360.0, 300.0)
KINDS = {"plain": (False, False), "nee": (True, False), "flagged": (True, True)}


def lamp_scene(kind, detail, w, h):
    """The scene with its emissive triangles removed and the lamp added."""
    sd = P.make_scene(kind, detail, 0x5EED0001, w, h)
    keep = sd.mats["emission"].sum(axis=1)[sd.tri_mat] == 0
    mat = np.zeros(1, sd.mats.dtype)
    mat[0]["kind"], mat[0]["emission"], mat[0]["ior"] = 0, EMISSION, 1.0
    return dataclasses.replace(sd, verts=sd.verts[keep], tri_mat=sd.tri_mat[keep], spheres=np.concatenate([sd.spheres, np.array([LAMP], np.float32)]),
                               sph_mat=np.concatenate([sd.sph_mat, np.array([len(sd.mats)], np.uint32)]), mats=np.concatenate([sd.mats, mat]))


def frame(r, w, h, spp, kind, seed=0x5EED0001, offset=0, acc=False):
    nee, sph = KINDS[kind]
    r.Params = P.make_params(w, h, spp=spp, max_depth=8, streams=8, seed=seed, flags=N.PT_FLAG_ACCUMULATE if acc else 0, sample_offset=offset,
                             next_event=nee, sphere_lights=sph)
    return r.Render(0.0)


def frames(r, kind, detail):
    out = {}
    r.SetScene(lamp_scene(kind, detail, 1920, 1080), 0)
    for k in KINDS:
        frame(r, 1920, 1080, 64, k)  # warm (allocation, first touch)
        st = [frame(r, 1920, 1080, 64, k) for _ in range(5)]
        ms = float(np.median([s.gpu_ms for s in st]))
        out[k] = {"ms": ms, "rays": int(st[0].rays), "grays_s": st[0].rays / ms / 1e6}
    for k in ("nee", "flagged"):
        out[k]["shadow_share"] = 1.0 - out["plain"]["rays"] / out[k]["rays"]
    w, h = 480, 270
    r.SetScene(lamp_scene(kind, detail, w, h), 0)
    for i in range(16):  # the converged frame: flagged, another seed, progressive
        frame(r, w, h, 512, "flagged", seed=77, offset=512 * i, acc=i > 0)
    ref = r.ReadFramebuffer()[..., :3].astype(np.float64)
    for k in KINDS:
        frame(r, w, h, 64, k)
        st = [frame(r, w, h, 64, k) for _ in range(3)]
        img = r.ReadFramebuffer()[..., :3].astype(np.float64)
        out[k]["small_ms"], out[k]["rmse"] = float(np.median([s.gpu_ms for s in st])), float(np.sqrt(np.mean((img - ref) ** 2)))
    f = out["flagged"]
    for k in ("plain", "nee"):
        out[k]["time_to_equal_error"] = (out[k]["rmse"] ** 2 * out[k]["small_ms"]) / (f["rmse"] ** 2 * f["small_ms"])
        out[k]["rmse_ratio_equal_spp"] = out[k]["rmse"] / f["rmse"]
    return out


def gathers(r, kind, detail, seeds=8):
    import torch
    from exp_gather import EPS, H, K, SEED, W, first_hit_points
    sd = lamp_scene(kind, detail, W, H)
    r.SetScene(sd, 0)
    p, n = first_hit_points(r, sd.cam)
    dp, dn = torch.from_numpy(p).cuda(), torch.from_numpy(n).cuda()
    torch.cuda.synchronize()
    bake = lambda sph, seed: r.GatherPaths(dp, dn, samples=K, seed=seed, ray_eps=EPS, max_depth=8, rr_start=3, next_event=True, sphere_lights=sph)
    ms = {False: [], True: []}
    rays = {}
    for rep in range(7):
        for sph in (False, True):
            st = bake(sph, SEED)[3]
            rays[sph] = int(st.rays)
            if rep >= 2:
                ms[sph].append(st.gpu_ms)
    out = {"points": len(p), "samples": K}
    for sph in (False, True):
        s1 = torch.zeros((len(p), 3), dtype=torch.float64, device="cuda")
        s2 = torch.zeros_like(s1)
        for j in range(seeds):
            E = torch.as_tensor(bake(sph, SEED + j)[0], device="cuda").double()
            s1 += E
            s2 += E * E
        var = float(((s2 - s1 * s1 / seeds) / (seeds - 1)).sum(1).mean())
        out["flagged" if sph else "nee"] = {"ms": float(np.median(ms[sph])), "rays": rays[sph], "variance": var}
    a, b = out["nee"], out["flagged"]
    out["efficiency_ratio"] = (a["variance"] * a["ms"]) / (b["variance"] * b["ms"])
    return out


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    names = [a for a in sys.argv[1:] if not a.startswith("--") and a != out_path]
    which = names[0].split(",") if names else list(SCENES)
    r = P.Renderer(P.Window(1920, 1080))
    r.Init()
    res = {}
    try:
        for name in which:
            res[name] = {"frames": frames(r, *SCENES[name])}
            print(name, "frames", json.dumps(res[name]["frames"]), flush=True)
            res[name]["gathers"] = gathers(r, *SCENES[name])
            print(name, "gathers", json.dumps(res[name]["gathers"]), flush=True)
    finally:
        r.Dispose()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
