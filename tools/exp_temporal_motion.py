"""Experiment: PT_TEMPORAL_MOTION (docs/SPEC.md §9.1) — what the motion pass costs beside the unchanged k_temporal and what it buys on a
moving object; the tables of DESIGN.md §12.1.

(1) cpu: the quality experiment on the oracle's frames with the scalar checkers (no GPU): Cornell with an object that comes closer under
    a still camera, 96x72, 8 frames of 1 spp, the default §8.2 filter over the accumulated image of the unflagged and of the flagged
    sequence, displayed RMSE over the object's pixels against a 2048-spp oracle frame of the last geometry.
(2) cost at 1920x1080: shade_ms of the flagged pass beside the unflagged k_temporal on the same frames (same geometry, seeds and
    updates), one à-trous pass of the same call beside them; median [min, max] of REPS calls after two warm-up calls. Cases: nothing
    moved (no update between the calls: the flagged call launches k_temporal; and an update to the same vertices: every pixel goes
    through the motion pass and is unmoved), one object moved (share of moved pixels from reserved[0]), every vertex of the 1M-triangle
    tessellated box moved by a small wave. Then the time of a device-to-device copy of the 1M-triangle snapshot's size (36 B per
    triangle), by device events around the copy.
(3) quality on the device: the experiment of (1) at 320x240 against a 4096-spp device frame.
usage: python tools/exp_temporal_motion.py [--reps 7] [--only cpu|cost|quality]"""
import argparse
import dataclasses
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, d)
import pathtracing_amd as P  # noqa: E402
import motion_cases as mc  # noqa: E402  (test infrastructure: the object, its motion and the error measure the tests use)

N = P.native
W, H = 1920, 1080


def mrange(xs):
    xs = sorted(xs)
    return f"{np.median(xs):7.4f} [{xs[0]:.4f}, {xs[-1]:.4f}]"


def cpu():
    import denoise_checker as dc
    import motion_checker as mr
    import pto
    dc.build()
    mr.build()
    q = mc.oracle_quality(P, pto, dc, mr)
    d = q["display"]
    print("== checker, 96x72, 8 frames of 1 spp, displayed RMSE over the object's pixels against 2048 spp")
    a = q["accumulated"]
    print(f"  filtered: unflagged {d[0]:.4f} -> flagged {d[1]:.4f} (ratio {d[1] / d[0]:.3f})   before the filter: {a[0]:.4f} -> {a[1]:.4f} "
          f"(ratio {a[1] / a[0]:.3f})   object pixels {q['pixels']}, moved in the last call {q['moved']}")


def waved(verts, phase):
    """Every vertex displaced by a small wave of its own position (shared vertices stay shared)."""
    v = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    d = 0.002 * np.sin(9.0 * v[:, [1, 2, 0]] + phase)
    return (v + d).astype(np.float32).reshape(-1, 9)


def cost_case(r, label, sd, geometry, reps, bvh=0):
    """geometry(k) -> SceneData of call k, or None for no update before call k."""
    res = {}
    for motion in (False, True):
        r.SetScene(sd, bvh)
        t, f, moved, took = [], [], [], []
        for k in range(reps + 2):
            g = geometry(k)
            if g is not None and k:
                r.UpdateGeometry(verts=g.verts)
            r.Params = P.make_params(W, H, spp=1, max_depth=8, seed=1000 + k)
            r.Render(0.0)
            st = r.DenoiseTemporal(iterations=1, reset=k == 0, motion=motion)
            if k >= 2:
                t.append(st.shade_ms); f.append(st.other_ms); moved.append(st.reserved[0] / float(W * H)); took.append(st.paths / float(W * H))
        res[motion] = (t, f, moved, took)
    (t0, f0, _, k0), (t1, _, m1, k1) = res[False], res[True]
    print(f"  {label:34s} k_temporal {mrange(t0)}  flagged {mrange(t1)}  one a-trous pass {mrange(f0)}  moved pixels {np.mean(m1):.3f}  "
          f"with history {np.mean(k0):.3f} -> {np.mean(k1):.3f}")


def cost(r, reps):
    print("== cost at 1920x1080 (shade_ms: median [min, max])")
    sd = mc.with_object(P, P.make_scene(N.PT_SCENE_CORNELL, 0, 0x5EED0001, W, H))
    cost_case(r, "nothing moved, no update", sd, lambda k: None, reps)
    cost_case(r, "nothing moved, same vertices", sd, lambda k: sd, reps)
    cost_case(r, "one object moved", sd, lambda k: mc.move_object(sd, (0.0, 0.0, 0.03 * k)), reps)
    big = P.make_scene(N.PT_SCENE_CORNELL_TESS, 1000000, 0x5EED0001, W, H)
    cost_case(r, f"every vertex of {len(big.tri_mat)} triangles", big, lambda k: dataclasses.replace(big, verts=waved(big.verts, 0.7 * k)), reps,
              N.PT_BVH_WIDTH_4Q | N.PT_BVH_BUILD_LBVH)
    import torch
    n = len(big.tri_mat) * 9
    src, dst = torch.zeros(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda")
    ms = []
    for k in range(reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); dst.copy_(src); b.record()
        torch.cuda.synchronize()
        if k >= 2:
            ms.append(a.elapsed_time(b))
    print(f"  device-to-device copy of {n * 4 / 1e6:.1f} MB (the snapshot of {len(big.tri_mat)} triangles): {mrange(ms)} ms")


def quality(r):
    print("== quality on the device, 320x240, 8 frames of 1 spp, displayed RMSE over the object's pixels against 4096 spp")
    q = mc.device_quality(P, r, 320, 240)
    d = q["display"]
    a = q["accumulated"]
    print(f"  filtered: unflagged {d[0]:.4f} -> flagged {d[1]:.4f} (ratio {d[1] / d[0]:.3f})   before the filter: {a[0]:.4f} -> {a[1]:.4f} "
          f"(ratio {a[1] / a[0]:.3f})   object pixels {q['pixels']}, moved in the last call {q['moved']}")


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
