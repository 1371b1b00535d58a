"""Experiment: pt_trace_rays rates (docs/SPEC.md §4.2) next to the extend kernel they share a traversal with. GPU only.

For the 1M-triangle tessellated Cornell box (BVH4Q), the 1M-triangle soup (BVH4Q) and plain Cornell (BVH2), two ray sets of device
records: coherent = the 1920x1080 camera rays; incoherent = from those rays' primary hits, cosine-distributed unit directions about
the surface normal (fixed seed), origins offset by ray_eps along the normal. Each set is traced as closest-hit and as occlusion
queries; a rate = rays / summed pt_stats.gpu_ms over repeated calls (>= 0.25 s of GPU time per repetition, 5 repetitions after
a warm-up), reported as median [min, max] Mrays/s. Yardstick, same scene and process: k_extend<L,false,-1> of a split-kernel
frame (PT_FLAG_SPLIT_KERNELS | PT_FLAG_PROFILE_KERNELS | PT_FLAG_EXTEND_SIMPLE, 1080p, 8 spp, depth 8, 8 streams): rays /
pt_stats.extend_ms, median [min, max] of 5 frames.
usage: python tools/exp_trace.py"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pathtracing_amd as P  # noqa: E402

N = P.native
W, H, EPS, REPS = 1920, 1080, 1e-4, 5


def camera_records(cam):
    """SPEC §3 camera rays of every pixel (pixel centres), vectorised: o | inf, normalize(forward + sx right + sy up) | 0."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    sx, sy = (x + 0.5) * cam.scale - cam.cx, (y + 0.5) * cam.scale - cam.cy
    f, r, u = (np.array(v[:], np.float32) for v in (cam.forward, cam.right, cam.up))
    d = (f + sx[..., None] * r + sy[..., None] * u).reshape(-1, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rec = np.zeros((len(d), 8), np.float32)
    rec[:, 0:3], rec[:, 3], rec[:, 4:7] = np.array(cam.origin[:], np.float32), np.inf, d
    return rec


def bounce_records(sd, rec, hits, seed=7):
    """Cosine-distributed directions about the normal at every primary hit (misses dropped), origins offset by EPS."""
    ids = np.ascontiguousarray(hits[:, 1]).view(np.uint32).astype(np.int64)
    ok = ids != 0xFFFFFFFF
    o, d, t, ids = rec[ok, 0:3], rec[ok, 4:7], hits[ok, 0:1], ids[ok]
    p = o + t * d
    v = np.asarray(sd.verts, np.float32).reshape(-1, 3, 3)
    nt = len(v)
    n = np.zeros_like(p)
    tri = ids < nt
    n[tri] = np.cross(v[ids[tri], 1] - v[ids[tri], 0], v[ids[tri], 2] - v[ids[tri], 0])
    sph = np.asarray(sd.spheres, np.float32).reshape(-1, 4)
    if (~tri).any():
        n[~tri] = p[~tri] - sph[ids[~tri] - nt, :3]
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n *= np.where((n * d).sum(1) < 0, 1.0, -1.0)[:, None].astype(np.float32)
    rng = np.random.default_rng(seed)
    u1, u2 = rng.random(len(p)), rng.random(len(p))
    a = np.where(np.abs(n[:, :1]) > 0.9, [[0, 1, 0]], [[1, 0, 0]]).astype(np.float32)
    tx = np.cross(n, a); tx /= np.linalg.norm(tx, axis=1, keepdims=True)
    ty = np.cross(n, tx)
    r, phi = np.sqrt(u1)[:, None], (2 * np.pi * u2)[:, None]
    dd = r * np.cos(phi) * tx + r * np.sin(phi) * ty + np.sqrt(1 - u1)[:, None] * n
    dd /= np.linalg.norm(dd, axis=1, keepdims=True)
    out = np.zeros((len(p), 8), np.float32)
    out[:, 0:3], out[:, 3], out[:, 4:7] = p + EPS * n, np.inf, dd
    return out


def spread(xs):
    xs = sorted(xs)
    return f"{xs[len(xs) // 2]:9.1f} [{xs[0]:.1f}, {xs[-1]:.1f}]"


def query_rate(r, rays, occlusion):
    for _ in range(2):
        r.TraceRays(rays, occlusion=occlusion)
    rates = []
    for _ in range(REPS):
        n, ms = 0, 0.0
        while ms < 250.0:
            _, st = r.TraceRays(rays, occlusion=occlusion)
            n, ms = n + st.rays, ms + st.gpu_ms
        rates.append(n / ms / 1e3)
    return rates


def extend_rate(r):
    r.Params = P.make_params(W, H, spp=8, max_depth=8, streams=8,
                             flags=N.PT_FLAG_SPLIT_KERNELS | N.PT_FLAG_PROFILE_KERNELS | N.PT_FLAG_EXTEND_SIMPLE)
    for _ in range(2):
        r.Render(0.0)
    return [st.rays / st.extend_ms / 1e3 for st in (r.Render(0.0) for _ in range(REPS))]


def main():
    r = P.Renderer(P.Window(W, H))
    r.Init()
    try:
        print(f"{'scene':8s} {'layout':>6s} {'rays':>8s}  {'closest Mrays/s':>26s}  {'occlusion Mrays/s':>26s}  {'k_extend<L,false,-1> Mrays/s':>28s}")
        for name, kind, detail in (("tess", N.PT_SCENE_CORNELL_TESS, 1 << 20), ("soup", N.PT_SCENE_TRIANGLE_SOUP, 1 << 20),
                                   ("cornell", N.PT_SCENE_CORNELL, 0)):
            sd = P.make_scene(kind, detail, 0x5EED0001, W, H)
            r.SetScene(sd, 0)
            layout = r.BvhInfo().width
            ext = spread(extend_rate(r))
            coherent = camera_records(sd.cam)
            hits, _ = r.TraceRays(coherent)
            for set_name, rec in (("coherent", coherent), ("incoherent", bounce_records(sd, coherent, hits))):
                dev = torch.from_numpy(rec).cuda()
                print(f"{name:8s} {layout:6d} {len(rec):8d}  {set_name:10s} {spread(query_rate(r, dev, False))}  "
                      f"{spread(query_rate(r, dev, True)):>26s}  {ext:>28s}", flush=True)
    finally:
        r.Dispose()


if __name__ == "__main__":
    main()
