"""Experiment: pt_scene_update_triangles (docs/SPEC.md §4.3) next to pt_scene_commit, and what refitting costs the frame. GPU only.

(1) Update times. For the 1M-triangle tessellated Cornell box (host SAH BVH4Q and GPU LBVH BVH4Q) and the 1M-triangle soup (both
    builders, BVH4Q): pt_scene_update_triangles from a numpy array (staged) and from a torch device tensor, each as pt_stats.gpu_ms
    and as wall time of the call; next to the wall time of pt_scene_commit on the same geometry. Median [min, max] of REPS calls
    after two warm-up calls; the updates alternate between two deformed copies of the mesh, so that every call moves the geometry.
(2) Traversal cost of refitting. The headline frame (1920x1080, 64 spp, depth 8, 8 streams) of the 1M-triangle Cornell box,
    committed with the host SAH builder (BVH4Q), after a smooth deformation y += a * extent * sin(8 x / extent + 5 z / extent) of
    increasing amplitude a: frame gpu_ms with the refitted tree and with a fresh commit of the same vertices (median [min, max] of
    REPS frames after a warm-up frame; the one-ray-per-lane extend kernel forced by pt_tuning.extend_kernel, so that both trees run
    the same kernel), node visits per ray (a PT_FLAG_COUNT_VISITS frame of 4 spp) and sah_cost of both.
usage: python tools/exp_refit.py [--reps 5] [--only updates|frames]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pathtracing_amd as P  # noqa: E402

N = P.native
W, H = 1920, 1080


def mrange(xs):
    xs = sorted(xs)
    return f"{np.median(xs):8.3f} [{xs[0]:.3f}, {xs[-1]:.3f}]"


def wave(verts, a):
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    ext = float(np.ptp(v, axis=0).max())
    out = v.astype(np.float64)
    out[:, 1] += a * ext * np.sin(8.0 * v[:, 0] / ext + 5.0 * v[:, 2] / ext)
    return out.astype(np.float32).reshape(-1, 9)


def updates(r, reps):
    print("== update vs commit (ms: median [min, max])")
    for label, kind, width in (("cornell 1M  SAH  4Q", N.PT_SCENE_CORNELL_TESS, 68), ("cornell 1M  LBVH 4Q", N.PT_SCENE_CORNELL_TESS, 68 | N.PT_BVH_BUILD_LBVH),
                               ("soup 1M     SAH  4Q", N.PT_SCENE_TRIANGLE_SOUP, 68), ("soup 1M     LBVH 4Q", N.PT_SCENE_TRIANGLE_SOUP, 68 | N.PT_BVH_BUILD_LBVH)):
        sd = P.make_scene(kind, 1_000_000, 0x5EED0001, W, H)
        commit = []
        for k in range(reps + 1):
            t0 = time.perf_counter()
            r.SetScene(sd, width)
            dt = (time.perf_counter() - t0) * 1e3
            if k:
                commit.append(dt)
        host = [wave(sd.verts, 0.01), wave(sd.verts, -0.01)]
        dev = [torch.from_numpy(v).cuda() for v in host]
        torch.cuda.synchronize()
        res = {}
        for name, arrs in (("host", host), ("device", dev)):
            gpu, wall = [], []
            for k in range(reps + 2):
                t0 = time.perf_counter()
                st = r.UpdateGeometry(verts=arrs[k % 2])
                dt = (time.perf_counter() - t0) * 1e3
                if k >= 2:
                    gpu.append(st.gpu_ms); wall.append(dt)
            res[name] = (gpu, wall)
        info = r.BvhInfo()
        print(f"{label}: n_nodes {info.n_nodes}, levels {info.max_depth}")
        print(f"   commit wall            {mrange(commit)}")
        for name in ("host", "device"):
            print(f"   update {name:6s} gpu_ms    {mrange(res[name][0])}")
            print(f"   update {name:6s} wall      {mrange(res[name][1])}")
        sys.stdout.flush()


def frames(r, reps):
    print("== headline frame after a deformation: refitted vs fresh commit (SAH BVH4Q)")
    sd = P.make_scene(N.PT_SCENE_CORNELL_TESS, 1_000_000, 0x5EED0001, W, H)
    params = P.make_params(W, H, spp=64, max_depth=8, streams=8)

    r.SetTuning(extend_kernel=1)

    def timed():
        r.Params = params
        r.Render(0.0)
        ms = [r.Render(0.0).gpu_ms for _ in range(reps)]
        r.Params = P.make_params(W, H, spp=4, max_depth=8, streams=8, flags=N.PT_FLAG_COUNT_VISITS)
        st = r.Render(0.0)
        return ms, st.node_visits / st.rays

    for a in (0.0, 0.001, 0.01, 0.03, 0.1, 0.3):
        v = wave(sd.verts, a)
        r.SetScene(sd, 68)
        r.UpdateGeometry(verts=v)
        (refit_ms, refit_nv), refit_sah = timed(), r.BvhInfo().sah_cost
        r.SetScene(P.SceneData(verts=v, tri_mat=sd.tri_mat, spheres=sd.spheres, sph_mat=sd.sph_mat, mats=sd.mats, cam=sd.cam, sky=sd.sky), 68)
        (fresh_ms, fresh_nv), fresh_sah = timed(), r.BvhInfo().sah_cost
        print(f"a = {a:5.3f}: refit {mrange(refit_ms)} ms  {refit_nv:6.2f} nodes/ray  sah {refit_sah:8.2f} | "
              f"fresh {mrange(fresh_ms)} ms  {fresh_nv:6.2f} nodes/ray  sah {fresh_sah:8.2f} | ratio {np.median(refit_ms) / np.median(fresh_ms):.3f}")
        sys.stdout.flush()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=("updates", "frames"), default=None)
    args = ap.parse_args()
    r = P.Renderer(P.Window(W, H))
    r.Init()
    try:
        if args.only in (None, "updates"):
            updates(r, args.reps)
        if args.only in (None, "frames"):
            frames(r, args.reps)
    finally:
        r.Dispose()
