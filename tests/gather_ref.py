"""docs/SPEC.md §12 (pt_gather) restated on the CPU, for tests only.

Nothing here transcribes the sampling code: the key and the random numbers are the oracle's pto_path_key / pto_u01, the direction is
pto_bsdf_sample with a Lambert material, occlusion is the oracle's closest hit (pto.Scene.closest) under §4.2's `t <= tmax` rule, as
spec_trace of tests/test_trace_rays.py does it, and an environment texel is env_checker.encode's. What is restated is §12's own text: the
unit normal, the origin offset, the three sums (in float64: the tests' tolerance is the bound of an f32 sum in any order) and the
invalid-point rule.

`rays` makes the n * K rays of a point set once (the slow part: two oracle calls per ray); `gather` turns them into the reference
outputs for a max_distance and a sky or map. `first_hits` makes the point sets the tests use: the first hits of a camera frame, from the
float64 caster, with the geometric normal turned towards the camera."""
import ctypes as C
import dataclasses
import math

import numpy as np

import env_checker
import ray_caster64 as rc

MISS = 0xFFFFFFFF
F3 = C.c_float * 3
K, EPS, W, H = 64, 1e-3, 24, 18  # the tests' samples per point, ray_eps and frame


def _f32(x):
    return np.float32(x)


def unit_normal(n):
    """§0's normalize on one f32 vector: s = 1 / sqrt(fma(z, z, fma(y, y, x * x))), then three products."""
    x, y, z = (float(_f32(c)) for c in n)
    dot = float(_f32(z * z + float(_f32(y * y + float(_f32(x * x))))))  # products of two f32 are exact in f64
    s = _f32(1.0) / _f32(math.sqrt(dot))
    return np.array([_f32(x) * s, _f32(y) * s, _f32(z) * s], np.float32)


def valid_point(p, n):
    p, n = np.asarray(p, np.float32), np.asarray(n, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        n2 = unit_dot(n)
    return bool(np.isfinite(p).all() and np.isfinite(n).all() and np.isfinite(n2) and n2 > 0)


def unit_dot(n):
    x, y, z = (float(c) for c in n)
    return float(_f32(z * z + float(_f32(y * y + float(_f32(x * x))))))


@dataclasses.dataclass
class Rays:
    valid: np.ndarray  # (n,) bool
    o: np.ndarray      # (n, 3) f32 origins (zeros for invalid points)
    d: np.ndarray      # (n, K, 3) f32 unit directions
    ids: np.ndarray    # (n, K) uint64: the oracle's closest hit, MISS for none
    t: np.ndarray      # (n, K) f32: its distance


def rays(P, pto, osc, points, normals, samples=K, seed=0, sample_offset=0, point_offset=0, ray_eps=EPS):
    """The rays of §12 for every (point, sample) and the oracle's unbounded closest hit along each. (pto_path_key hashes the seed itself.)"""
    lam = np.zeros(1, P.MATERIAL_DTYPE)
    lam["kind"], lam["albedo"], lam["ior"] = 0, (1.0, 1.0, 1.0), 1.0
    mp = lam.ctypes.data_as(C.c_void_p)
    n_pts = len(points)
    out = Rays(np.zeros(n_pts, bool), np.zeros((n_pts, 3), np.float32), np.zeros((n_pts, samples, 3), np.float32),
               np.full((n_pts, samples), MISS, np.uint64), np.full((n_pts, samples), np.inf, np.float32))
    wi, Wt, side = F3(), F3(), C.c_float()
    eps = float(_f32(ray_eps))
    for i in range(n_pts):
        if not valid_point(points[i], normals[i]):
            continue
        out.valid[i] = True
        nn = unit_normal(normals[i])
        o = np.array([_f32(eps * float(nn[c]) + float(_f32(points[i][c]))) for c in range(3)], np.float32)  # fma(ray_eps, nn, p)
        out.o[i] = o
        nf = F3(*nn.tolist())
        for k in range(samples):
            key = pto.lib.pto_path_key(seed & 0xFFFFFFFF, (point_offset + i) & 0xFFFFFFFF, (sample_offset + k) & 0xFFFFFFFF)
            alive = pto.lib.pto_bsdf_sample(mp, F3(0.0, 0.0, 0.0), nf, 1, pto.lib.pto_u01(key, 0), pto.lib.pto_u01(key, 1), 0.0, wi, Wt, C.byref(side))
            assert alive == 1, f"pto_bsdf_sample refused a Lambert sample: point {i}, sample {k}, returned {alive}"
            out.d[i, k] = wi[:]
            out.ids[i, k], out.t[i, k] = osc.closest(o, out.d[i, k])
    return out


def visible(r, max_distance=0.0):
    """V (n, K) bool: no hit with t <= tmax (tmax = max_distance, +inf for 0). Rows of invalid points are all False."""
    tmax = np.float32(max_distance) if max_distance > 0 else np.float32(np.inf)
    return r.valid[:, None] & ~((r.ids != MISS) & (r.t <= tmax))


def radiance(r, sky=None, env=None):
    """L (n, K, 3) float64 of every direction: the map's texel at §11's encode(d), or the constant sky."""
    n_pts, samples = r.d.shape[:2]
    if env is None:
        return np.broadcast_to(np.asarray(sky, np.float32).astype(np.float64), (n_pts, samples, 3)).copy()
    env = np.asarray(env, np.float32)
    L = np.zeros((n_pts, samples, 3))
    for i in np.nonzero(r.valid)[0]:
        for k in range(samples):
            col, row, _ = env_checker.encode(r.d[i, k], env.shape[0])
            L[i, k] = env[row, col]
    return L


def gather(r, max_distance=0.0, sky=None, env=None, L=None):
    """The §12 outputs in float64: count (n,) int, visibility, E (n, 3), bent (n, 3) and absE = sum |V L| / K (the scale of E's bound).
    Invalid points: visibility -1, everything else 0."""
    samples = r.d.shape[1]
    V = visible(r, max_distance)
    if L is None:
        L = radiance(r, sky, env)
    Vf = V.astype(np.float64)[..., None]
    count = V.sum(1).astype(np.int64)
    vis = np.where(r.valid, count / samples, -1.0)
    E = (Vf * L).sum(1) / samples
    absE = (Vf * np.abs(L)).sum(1) / samples
    bent = (Vf * r.d.astype(np.float64)).sum(1) / samples
    return dict(count=count, visibility=vis, E=E, absE=absE, bent=bent, V=V)


def first_hits(P, pto, sd, w=W, h=H, step=1):
    """(points, normals) f32 of the first hits of a w x h camera frame of `sd`, from the float64 caster: the hit point and the geometric
    normal of the primitive, turned against the camera ray. Pixels that miss are left out. step: the camera is that of a frame of
    w * step x h * step pixels, of which every step-th of a row and of a column is taken (w x h points over the whole view)."""
    o, d = rc.camera_rays(pto, sd.cam, w * step, h * step)
    keep = (np.arange(h)[:, None] * step * (w * step) + np.arange(w)[None, :] * step).ravel()
    o, d = o[keep], d[keep]
    ids, t, _, _ = rc.cast(sd.verts, sd.spheres, o, d)
    hit = ids != MISS
    o64, d64 = o.astype(np.float64)[hit], d.astype(np.float64)[hit]
    p = o64 + t[hit, None] * d64
    v = np.asarray(sd.verts, np.float32).reshape(-1, 3, 3).astype(np.float64)
    sph = np.asarray(sd.spheres, np.float32).reshape(-1, 4).astype(np.float64)
    n = np.zeros_like(p)
    for j, pid in enumerate(ids[hit].astype(np.int64)):
        n[j] = np.cross(v[pid, 1] - v[pid, 0], v[pid, 2] - v[pid, 0]) if pid < len(v) else p[j] - sph[pid - len(v), :3]
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n[(n * d64).sum(1) > 0] *= -1.0
    return p.astype(np.float32), n.astype(np.float32)


def both_sides(points, normals):
    """The points, then the same points with the normal negated: that hemisphere looks into the surface's far side and ray_eps puts
    the origin behind the primitive, whose own back is then the first candidate."""
    return np.concatenate([points, points]), np.concatenate([normals, -np.asarray(normals, np.float32)])


def probe(cam, n=64, spread=0.25, seed=5):
    """`n` points on and around a camera's origin (the first is the origin itself, the rest within `spread` of it along every axis)
    with the camera's forward direction as normal: points that lie on no surface, for scenes whose first hits all look back at the
    camera."""
    rng = np.random.default_rng(seed)
    o = np.array([cam.origin[i] for i in range(3)], np.float64)
    pts = o + rng.uniform(-spread, spread, (n, 3))
    pts[0] = o
    return pts.astype(np.float32), np.tile(np.array([cam.forward[i] for i in range(3)], np.float32), (n, 1))


def centroids(sd, every=16):
    """(points, normals) f32 on every `every`-th triangle of the scene: its centroid and its unit geometric normal, from float64."""
    v = np.asarray(sd.verts, np.float32).reshape(-1, 3, 3).astype(np.float64)[::every]
    n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    return v.mean(1).astype(np.float32), (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)


def tiled(points, normals, n):
    """The point set repeated cyclically up to `n` points (every index of a call has its own key: the records differ)."""
    idx = np.arange(n) % len(points)
    return np.ascontiguousarray(points[idx]), np.ascontiguousarray(normals[idx])


def records(points, normals):
    r = np.zeros((len(points), 8), np.float32)
    r[:, 0:3], r[:, 4:7] = points, normals
    return r


def cast_rays(sd, r):
    """The float64 caster over the rays of `r` (the slow part of the comparison; independent of max_distance)."""
    samples = r.d.shape[1]
    return rc.cast(sd.verts, sd.spheres, np.repeat(r.o, samples, axis=0), r.d.reshape(-1, 3))


def clear_rays(r, cast, max_distance=0.0):
    """From cast_rays' result: (occluded64 (n, K) bool, clear (n, K) bool). Clear: the hit not within 1e-5 of an edge, the ray not in a
    triangle's plane, and the hit not within 1e-4 relative of max_distance."""
    n_pts, samples = r.d.shape[:2]
    ids, t, edge, in_plane = cast
    hit = ids != MISS
    tmax = max_distance if max_distance > 0 else np.inf
    with np.errstate(invalid="ignore"):
        clear = ~in_plane & ~(hit & (edge < 1e-5))
        if max_distance > 0:
            clear &= ~(hit & (np.abs(t - tmax) <= 1e-4 * t))
    occluded = hit & (t <= tmax)
    return occluded.reshape(n_pts, samples), clear.reshape(n_pts, samples)


# ------------------------------------------------------------------------------------------------------------------------ shared cases
_CASES = {}


def scene(P, name):
    """glass: C4 (12 triangles, 4 spheres). tess: C5 with 2000 triangles. closed: C1 with its open front walled up, no spheres."""
    N = P.native
    if name == "glass":
        return P.make_scene(N.PT_SCENE_CORNELL_GLASS, 0, 3, W, H)
    if name == "tess":
        return P.make_scene(N.PT_SCENE_CORNELL_TESS, 2000, 3, W, H)
    if name == "closed":
        sd = P.make_scene(N.PT_SCENE_CORNELL, 0, 3, W, H)
        v = np.asarray(sd.verts, np.float32).reshape(-1, 3)
        lo, hi = v.min(0), v.max(0)
        z = hi[2]  # the camera looks down -z through the open side
        front = np.array([[lo[0], lo[1], z, hi[0], lo[1], z, hi[0], hi[1], z], [lo[0], lo[1], z, hi[0], hi[1], z, lo[0], hi[1], z]], np.float32)
        return dataclasses.replace(sd, verts=np.concatenate([np.asarray(sd.verts, np.float32).reshape(-1, 9), front]),
                                   tri_mat=np.concatenate([sd.tri_mat, sd.tri_mat[:1], sd.tri_mat[:1]]).astype(np.uint32),
                                   spheres=np.zeros((0, 4), np.float32), sph_mat=np.zeros(0, np.uint32))
    raise KeyError(name)


def half_box(sd):
    """About half the scene's largest extent: the tests' finite max_distance."""
    v = np.asarray(sd.verts, np.float32).reshape(-1, 3)
    return float(np.float32(0.5 * (v.max(0) - v.min(0)).max()))


_SPACE = {}


def space_case(P, pto, name):
    """(scene, points, normals, ray_eps) of a scene of trace_support.scenes or a case of geometry_space (both have cameras of 48 x 36
    frames), made once per process and never written to. `layers`: the probe set on the camera origin (the first hits of the stacked
    layers all lie on the nearest one and look back at the camera). The other scenes of trace_support: the first hits of 24 x 18 pixels
    over the whole view, from both sides; the camera of `soup` sees few triangles between the gaps (4 of 432 pixels hit one), so its set
    goes on with the centroid of every 16th triangle, from both sides. A geometry_space case: those first hits, and the case's own
    ray_eps."""
    if name not in _SPACE:
        import geometry_space
        import trace_support
        if name == "layers":
            sd = trace_support.scenes(P)[name]
            _SPACE[name] = (sd,) + probe(sd.cam) + (EPS,)
        elif name in ("duplicates", "soup", "spheres64", "glass", "tess", "cornell"):
            sd = trace_support.scenes(P)[name]
            pts, nrm = first_hits(P, pto, sd, step=2)
            if name == "soup":
                more = centroids(sd)
                pts, nrm = np.concatenate([pts, more[0]]), np.concatenate([nrm, more[1]])
            _SPACE[name] = (sd,) + both_sides(pts, nrm) + (EPS,)
        else:
            c = geometry_space.cases()[name]
            _SPACE[name] = (c.sd,) + first_hits(P, pto, c.sd, step=2) + (float(np.float32(c.ray_eps)),)
    return _SPACE[name]


def tight_eps(sd):
    """32 ulps of the scene's largest |coordinate|: a ray_eps that keeps the origins next to their surfaces at large offsets, where a
    geometry_space case's own (1e-4 of the offset) carries them out of a box two units across."""
    v = np.asarray(sd.verts, np.float32)
    return float(32 * np.spacing(np.abs(v).max()))


def spread(points, normals, n=64):
    """`n` of the points, evenly spread over the set (the Python ray loop of `rays` is slow)."""
    idx = np.unique(np.linspace(0, len(points) - 1, n).astype(np.int64))
    return points[idx], normals[idx]


def case(P, pto, name, samples=K):
    """(scene, points, normals, Rays with `samples` samples, seed 0, offsets 0, ray_eps EPS) of the first hits of the W x H frame, made
    once per process and never written to."""
    key = (name, samples)
    if key not in _CASES:
        from float64_support import build_bvh_detached
        sd = scene(P, name)
        info, nodes, tris = build_bvh_detached(sd, 68)
        osc = pto.Scene(sd, (info.width, nodes, tris))
        pts, nrm = first_hits(P, pto, sd)
        _CASES[key] = (sd, pts, nrm, rays(P, pto, osc, pts, nrm, samples))
    return _CASES[key]
