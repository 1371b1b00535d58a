"""What the ray-query tests share: the layouts and the miss id of the test side, the 48 x 36 scene dictionary, ray sets, ray records,
the oracle's closest hit over a batch, and the comparison of the device's hit records with it. Test helpers only.

LAYOUTS and MISS are stated here once for the tests. The references (ray_caster64, denoise64, the *_checker bindings) restate the
spec on their own and keep their own MISS."""
import ctypes as C

import numpy as np

import adversarial_scenes as S
import ray_caster64 as rc

LAYOUTS = [2, 4, 68, 72, 73]
MISS = 0xFFFFFFFF
W, H = 48, 36


def scenes(P):
    N = P.native
    return {
        "cornell": P.make_scene(N.PT_SCENE_CORNELL, 0, 3, W, H),
        "glass": P.make_scene(N.PT_SCENE_CORNELL_GLASS, 0, 3, W, H),
        "tess": P.make_scene(N.PT_SCENE_CORNELL_TESS, 3000, 3, W, H),
        "soup": P.make_scene(N.PT_SCENE_TRIANGLE_SOUP, 4000, 3, W, H),
        "layers": S.stacked_layers(W, H),
        "duplicates": S.duplicates(W, H)[0],
        "spheres64": S.sphere_list(64, W, H),
    }


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def ray_sets(pto, sd, n=600, seed=11):
    """(name, origins, directions): camera rays, rays with exactly-zero direction components, incoherent unit rays from inside the
    scene's bounds, and rays that start on surfaces."""
    rng = np.random.default_rng(seed)
    o, d = rc.camera_rays(pto, sd.cam, W, H)
    pts = np.concatenate([np.asarray(sd.verts, np.float32).reshape(-1, 3), np.asarray(sd.spheres, np.float32).reshape(-1, 4)[:, :3]])
    lo, hi = pts.min(0), pts.max(0)
    inside = (lo + rng.random((n, 3)) * (hi - lo)).astype(np.float32)
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, 0.6, -0.8], [0.8, 0, 0.6], [-0.6, -0.8, 0]], np.float32)
    zero_d = axes[rng.integers(0, len(axes), n)]
    out = [("camera", o, d), ("zero_components", inside, zero_d), ("incoherent", inside[::-1].copy(), _unit(rng.normal(size=(n, 3))))]
    if len(sd.verts):
        v = np.asarray(sd.verts, np.float32).reshape(-1, 3, 3)
        k = rng.integers(0, len(v), n)
        a, b = rng.random(n), rng.random(n)
        flip = a + b > 1
        a[flip], b[flip] = 1 - a[flip], 1 - b[flip]
        on = (v[k, 0] + a[:, None] * (v[k, 1] - v[k, 0]) + b[:, None] * (v[k, 2] - v[k, 0])).astype(np.float32)
        out.append(("on_surface", on, _unit(rng.normal(size=(n, 3)))))
    return out


def records(o, d, tmax=np.inf):
    r = np.zeros((len(o), 8), np.float32)
    r[:, 0:3], r[:, 3], r[:, 4:7] = o, tmax, d
    return r


def oracle(pto, osc, o, d):
    """(ids uint64, t float32, summed pto_stats) of pto_closest over the rays."""
    st = pto.pto_stats()
    t = C.c_float()
    ids, ts = np.empty(len(o), np.uint64), np.empty(len(o), np.float32)
    fo, fd = C.c_float * 3, C.c_float * 3
    for i in range(len(o)):
        ids[i] = pto.lib.pto_closest(C.byref(osc.c), fo(*o[i].tolist()), fd(*d[i].tolist()), C.byref(t), C.byref(st))
        ts[i] = t.value
    return ids, ts, st


def same(a, b):
    """Hit records equal bit for bit (a miss's id bits are a NaN as a float)."""
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def ids_of(hits):
    return np.ascontiguousarray(hits[:, 1]).view(np.uint32).astype(np.uint64)


def commit(P, pto, r, sd, width):
    r.SetScene(sd, width)
    info = r.BvhInfo()
    osc = pto.Scene(sd, (info.width,) + r.BvhRead())
    assert osc.validate_bvh()[0] == 0, ("validate_bvh", osc.validate_bvh()[0], width)
    return osc


def check_closest(hits, ids, ts, ctx):
    got = ids_of(hits)
    assert np.array_equal(got, ids), (ctx, np.nonzero(got != ids)[0][:8])
    hit = ids != MISS
    assert np.array_equal(hits[hit, 0].view(np.uint32), ts[hit].view(np.uint32)), ctx
    assert (hits[~hit, 0] == np.inf).all() and (hits[~hit, 2:] == 0).all(), ctx
