"""A float64 ray caster: the closest hit of SPEC §4 computed independently of the f32 spec, for tests only.

The scene arrays and rays are float32, as the product and the oracle see them; they are widened to float64 exactly, so
the caster answers the geometric question for the very same inputs. Triangles use Möller–Trumbore on the vertices (edges
inclusive), spheres the well-conditioned discriminant `r² - |oc - b·d|²`. The closest hit is the lowest `(t, prim_id)`,
exactly as SPEC §4 defines it. Brute force, vectorised over rays × primitives in chunks.

`classify` sorts the disagreements of an f32 implementation (the device or the oracle) with the caster into the classes
float64 cannot settle — a ray within `EDGE_BAND` of an edge of either candidate (a miss there is a crack), candidates whose
`t` agree to `T_BAND` — and real disagreements, which a test expects to be none. The bands are arguments (scalars or one
value per ray) with these defaults. A sphere far away in its own radii has a third class of its own: SPEC §4's discriminant
`b² − (|oc|² − r²)` cancels, so its silhouette is uncertain by `K_S · (|oc|/r)² · 2^-24` of r² (`sphere_band`).

A triangle without area (`cross(e1, e2) == 0` in float64: a repeated vertex, collinear vertices, a point) is never hit and has
no plane for a ray to lie in.
"""
import numpy as np

MISS = 0xFFFFFFFF
EDGE_BAND = 1e-5  # barycentric units
T_BAND = 1e-5     # relative difference of t
_PAIRS = 1 << 19  # rays × primitives per chunk
# The scaled sphere band, in units of (|oc|/r)² · 2^-24 of r². Measured on the oracle over geometry_space's far_sphere and
# far_camera cases (tests/test_geometry_space.py test_k_s_is_twice_the_measured_value repeats the measurement): the largest
# |disc64|/r² / ((|oc|/r)² · 2^-24) among the rays that disagree with float64 is K_S_MEASURED; the band is twice that. The
# rounding argument (three roundings each in b·b, oc·oc and the fma, each half an ulp of |oc|² ~ 2^-24 |oc|²) allows about 4.5.
# At K_S the band is 1 % of r² at sqrt(0.01 · 2^24 / K_S) = 147 radii; at 3000 radii it is 4.2 r²: the test is noise there.
K_S_MEASURED = 3.89  # 3.884, on far_camera at 1000 units; far_sphere alone: 2.32
K_S = 2 * K_S_MEASURED


def camera_rays(pto, cam, width, height):
    """The camera rays of a width × height frame (SPEC §3, key 0), from the oracle: (R, 3) float32 origins and directions."""
    o = np.empty((height * width, 3), np.float32)
    d = np.empty((height * width, 3), np.float32)
    for y in range(height):
        for x in range(width):
            o[y * width + x], d[y * width + x] = pto.camera_ray(cam, x, y)
    return o, d


def _tri64(verts):
    v = np.asarray(verts, np.float32).reshape(-1, 3, 3).astype(np.float64)
    return v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]


def _tri_eval(o, d, v0, e1, e2):
    """Möller–Trumbore in float64 for rays (R,3) against triangles (R or 1, 3): t, u, v, det (all (R, T))."""
    p = np.cross(d, e2)
    det = np.einsum("...k,...k->...", e1, p)
    tv = o - v0
    q = np.cross(tv, e1)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / det
        u = np.einsum("...k,...k->...", tv, p) * inv
        v = np.einsum("...k,...k->...", d, q) * inv
        t = np.einsum("...k,...k->...", e2, q) * inv
    return t, u, v, det


def _sph_eval(o, d, c, r):
    """Ray-sphere in float64: t of the first intersection in front of the origin (NaN if none) and the discriminant over r²."""
    oc = o - c
    a = np.einsum("...k,...k->...", d, d)
    b = np.einsum("...k,...k->...", oc, d) / a
    perp = oc - b[..., None] * d
    disc = r * r - np.einsum("...k,...k->...", perp, perp)
    with np.errstate(invalid="ignore"):
        s = np.sqrt(disc / a)
        t0, t1 = -b - s, -b + s
        t = np.where(t0 > 0, t0, t1)
        t = np.where((disc > 0) & (t > 0), t, np.nan)
    return t, disc / (r * r)


def _edge(u, v):
    """Distance of a barycentric point to the nearest edge line: >= 0 inside, the largest violation outside."""
    with np.errstate(invalid="ignore"):
        return np.abs(np.minimum(np.minimum(u, v), 1.0 - u - v))


def _cross2(a, b):
    return a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]


def _meets_in_plane(o, d, v0, e1, e2):
    """For rays (K,3) lying in the planes of triangles (K,3 each): does the ray (s >= 0) touch the triangle? Worked in 2D after
    dropping the axis of the normal's largest component: the origin is inside, or the ray crosses or runs along an edge."""
    n = np.abs(np.cross(e1, e2))
    keep = np.array([[1, 2], [0, 2], [0, 1]])[np.argmax(n, axis=1)]
    pick = lambda x: np.take_along_axis(x, keep, axis=1)  # noqa: E731
    o2, d2 = pick(o), pick(d)
    p = [pick(v0), pick(v0 + e1), pick(v0 + e2)]
    side = [_cross2(p[(i + 1) % 3] - p[i], o2 - p[i]) for i in range(3)]
    meets = ((side[0] >= 0) & (side[1] >= 0) & (side[2] >= 0)) | ((side[0] <= 0) & (side[1] <= 0) & (side[2] <= 0))
    for i in range(3):
        a, e = p[i], p[(i + 1) % 3] - p[i]
        den = _cross2(d2, e)
        ao = a - o2
        with np.errstate(divide="ignore", invalid="ignore"):
            sr, w = _cross2(ao, e) / den, _cross2(ao, d2) / den
        crosses = (den != 0) & (sr >= 0) & (w >= 0) & (w <= 1)
        along = (den == 0) & (_cross2(ao, d2) == 0) & (((ao * d2).sum(-1) >= 0) | (((ao + e) * d2).sum(-1) >= 0))
        meets |= crosses | along
    return meets


def _rays(a, rays64):
    """Ray origins or directions as float64: through float32, as the product and the oracle see them, unless rays64 says that they are
    a float64 reference's own (tests/lens64.py), to be cast as they are."""
    return np.asarray(a, np.float64) if rays64 else np.asarray(a, np.float32).astype(np.float64)


def cast(verts, spheres, o, d, rays64=False):
    """Closest hit of every ray: (prim id or MISS as uint64, t float64, edge distance of the hit float64, in_plane bool).
    `in_plane`: the ray lies in the plane of a triangle it touches (det == 0, the origin in the plane, and the ray meets the
    triangle within that plane), where Möller–Trumbore has no answer; such rays are left out of every comparison. A ray that
    is merely coplanar with a triangle it never reaches is compared as usual."""
    o, d = _rays(o, rays64), _rays(d, rays64)
    R = len(o)
    best_t = np.full(R, np.inf)
    best_id = np.full(R, MISS, np.uint64)
    best_edge = np.full(R, np.nan)
    in_plane = np.zeros(R, bool)
    v0, e1, e2 = _tri64(verts)
    NT = len(v0)
    step_r = max(1, min(R, _PAIRS // max(NT, 1)))
    step_t = max(1, _PAIRS // step_r)
    for r0 in range(0, R, step_r):
        rs = slice(r0, r0 + step_r)
        oo, dd = o[rs, None], d[rs, None]
        for t0 in range(0, NT, step_t):
            ts = slice(t0, t0 + step_t)
            t, u, v, det = _tri_eval(oo, dd, v0[None, ts], e1[None, ts], e2[None, ts])
            with np.errstate(invalid="ignore"):
                ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)
            n = np.cross(e1[ts], e2[ts])
            off = np.einsum("rtk,tk->rt", oo - v0[None, ts], n)
            ri, ti = np.nonzero((det == 0) & (off == 0) & (n != 0).any(axis=1)[None, :])  # a zero-area triangle has no plane
            if len(ri):
                ti = ti + t0
                touch = _meets_in_plane(o[ri + r0], d[ri + r0], v0[ti], e1[ti], e2[ti])
                in_plane[ri[touch] + r0] = True
            tt = np.where(ok, t, np.inf)
            j = np.argmin(tt, axis=1)  # first minimum: the lowest id among equal t
            rows = np.arange(tt.shape[0])
            tj = tt[rows, j]
            better = tj < best_t[rs]  # chunks go in increasing id, so an equal t never replaces a lower id
            idx = np.nonzero(better)[0] + r0
            best_t[idx] = tj[better]
            best_id[idx] = (j[better] + t0).astype(np.uint64)
            best_edge[idx] = _edge(u[rows, j], v[rows, j])[better]
    sph = np.asarray(spheres, np.float32).reshape(-1, 4).astype(np.float64)
    for k, s in enumerate(sph):
        t, disc = _sph_eval(o, d, s[:3], s[3])
        better = t < best_t  # spheres have the highest ids: only a strictly smaller t wins
        best_t[better] = t[better]
        best_id[better] = NT + k
        best_edge[better] = np.abs(disc[better])
    return best_id, best_t, best_edge, in_plane


def candidate(verts, spheres, o, d, ids, rays64=False):
    """float64 t (NaN for a miss or a non-intersection) and edge distance of primitive ids[i] along ray i."""
    o, d = _rays(o, rays64), _rays(d, rays64)
    ids = np.asarray(ids, np.uint64)
    t = np.full(len(o), np.nan)
    edge = np.full(len(o), np.nan)
    v0, e1, e2 = _tri64(verts)
    NT = len(v0)
    tri = ids < NT
    if tri.any():
        j = ids[tri].astype(np.int64)
        tt, u, v, det = _tri_eval(o[tri], d[tri], v0[j], e1[j], e2[j])
        t[tri] = np.where(det != 0, tt, np.nan)
        edge[tri] = _edge(u, v)
    sph = np.asarray(spheres, np.float32).reshape(-1, 4).astype(np.float64)
    isph = (ids >= NT) & (ids != MISS)
    if isph.any():
        s = sph[(ids[isph] - NT).astype(np.int64)]
        tt, disc = _sph_eval(o[isph], d[isph], s[:, :3], s[:, 3])
        t[isph] = tt
        edge[isph] = np.abs(disc)
    return t, edge


def sphere_distance2(verts, spheres, o, ids, rays64=False):
    """(|oc|/r)² of ray i's origin to sphere ids[i], in float64; NaN where ids[i] is not a sphere."""
    o = _rays(o, rays64)
    ids = np.asarray(ids, np.uint64)
    NT = len(np.asarray(verts).reshape(-1, 9))
    sph = np.asarray(spheres, np.float32).reshape(-1, 4).astype(np.float64)
    out = np.full(len(o), np.nan)
    isph = (ids >= NT) & (ids != MISS)
    if isph.any():
        s = sph[(ids[isph] - NT).astype(np.int64)]
        oc = o[isph] - s[:, :3]
        out[isph] = (oc * oc).sum(-1) / (s[:, 3] * s[:, 3])
    return out


def classify(verts, spheres, o, d, got, cast_result=None, edge_band=EDGE_BAND, t_band=T_BAND, sphere_band=False, t_floor=None,
             rays64=False):
    """Compare the primitive ids `got` (uint, MISS for none) of an f32 implementation with the caster, ray by ray.
    Returns a dict of index arrays: agree, edge (near an edge of either candidate), crack (the edge rays where `got` misses),
    coincident (the two candidates' t agree to t_band), in_plane (left out), wrong (everything else). `cast_result`: what
    cast() returned for these rays, to skip recomputing it. `edge_band`, `t_band`: scalars or one value per ray. `sphere_band`:
    a candidate that is a sphere also counts as edge when |disc64|/r² <= K_S · (|oc|/r)² · 2^-24 (the cancellation of SPEC §4's
    discriminant); the dict then also holds `sphere_ratio`, |disc64|/r² over (|oc|/r)² · 2^-24 of the sphere candidate (the
    smaller of the two if both are spheres, NaN if neither is) for every ray. `t_floor` (a length, scalar or per ray; only for rays
    that start on a triangle): the start is a rounded point a few ulps off the triangle's plane, so whether that triangle S is hit at
    once, at a t of rounding size, is not for float64 to say. A disagreement goes to the class `origin` (always empty without t_floor)
    only if it is exactly that: either `got` is a triangle S with |t64| <= t_floor and the caster's answer is what the caster finds
    with S left out, or the caster's answer is such an S and `got` is what the caster finds with S left out. Any other id is judged
    as usual. `rays64`: o and d are float64 rays of a reference, cast as they are (the default widens float32 rays)."""
    got = np.asarray(got).astype(np.uint64)
    want, t_w, edge_w, in_plane = cast_result if cast_result is not None else cast(verts, spheres, o, d, rays64)
    t_g, edge_g = candidate(verts, spheres, o, d, got, rays64)
    agree = (got == want) & ~in_plane
    dis = (got != want) & ~in_plane
    extra = {}
    with np.errstate(invalid="ignore"):
        origin = np.zeros(len(got), bool)
        if t_floor is not None:
            NT = len(np.asarray(verts).reshape(-1, 9))
            floor = np.broadcast_to(np.asarray(t_floor, np.float64), got.shape)
            for i in np.nonzero(dis & (((np.abs(t_g) <= floor) & (got < NT)) | ((t_w <= floor) & (want < NT))))[0]:
                start = want[i] if t_w[i] <= floor[i] and want[i] < NT else got[i]  # the triangle the ray starts on
                rest = np.array(np.asarray(verts, np.float32).reshape(-1, 9), copy=True)
                rest[int(start)] = 0  # without area: never hit
                without = cast(rest, spheres, o[i:i + 1], d[i:i + 1], rays64)[0][0]
                origin[i] = (got[i] if start == want[i] else want[i]) == without
        dis = dis & ~origin
        near_edge = dis & ((edge_w < edge_band) | (edge_g < edge_band))
        if sphere_band:
            unit = 2.0 ** -24
            ratio = np.fmin(edge_w / (sphere_distance2(verts, spheres, o, want, rays64) * unit),
                            edge_g / (sphere_distance2(verts, spheres, o, got, rays64) * unit))
            near_edge |= dis & (ratio <= K_S)
            extra["sphere_ratio"] = ratio
        close_t = dis & ~near_edge & (np.abs(t_g - t_w) <= t_band * np.maximum(np.abs(t_g), np.abs(t_w)))
    wrong = dis & ~near_edge & ~close_t
    ix = np.nonzero
    return dict(agree=ix(agree)[0], edge=ix(near_edge)[0], crack=ix(near_edge & (got == MISS))[0], coincident=ix(close_t)[0],
                in_plane=ix(in_plane)[0], wrong=ix(wrong)[0], origin=ix(origin)[0], want=want, **extra)


def _node_slots(layout, nodes, i):
    """Child slots of node i of a SPEC §4.1 blob: list of (lo[3], hi[3], ref), empty slots dropped. Quantised boxes are decoded
    with the f32 expression of the spec, so they are the boxes the kernels test."""
    if layout in (2, 4):
        raw = nodes[i * 32 * layout:(i + 1) * 32 * layout]
        f = raw.view(np.float32).reshape(layout, 8)
        ref = raw.view(np.int32).reshape(layout, 8)[:, 3]
        return [(f[c, :3].astype(np.float64), f[c, 4:7].astype(np.float64), int(ref[c])) for c in range(layout) if ref[c] != 0x7FFFFFFF]
    n, size, ql = (4, 64, 32) if layout == 68 else (8, 128, 48)
    raw = nodes[i * size:(i + 1) * size]
    org = raw[:12].view(np.float32)
    sc = (raw[12:15].astype(np.uint32) << 23).view(np.float32)
    ref = raw[16:16 + 4 * n].view(np.int32)
    q = raw[ql:ql + 6 * n].reshape(6, n).astype(np.float32)
    out = []
    for c in range(n):
        if ref[c] == 0x7FFFFFFF:
            continue
        lo = (q[0:3, c] * sc + org).astype(np.float64)  # single rounding each: q * 2^e is exact, so this is the spec's fma
        hi = (q[3:6, c] * sc + org).astype(np.float64)
        out.append((lo, hi, int(ref[c])))
    return out


def stack_depth(layout, nodes, tris48, o, d, margin=1e-3):
    """Largest traversal-stack depth (entries held besides the current node, SPEC §4 push order) of one ray through the blob, walked in float64: t_best
    shrinks as the leaves' triangles are hit, boxes are shrunk by `margin` of their extent and a leaf's hit lowers t_best by
    the same fraction, so that a child this walk counts as hit is hit by the f32 traversal too."""
    tri = np.asarray(tris48, np.uint8).view(np.float32).reshape(-1, 12).astype(np.float64)
    t_best = np.inf
    o = np.asarray(o, np.float64)
    d = np.asarray(d, np.float64)
    with np.errstate(divide="ignore"):
        inv = 1.0 / d
    octant = int(inv[0] < 0) | int(inv[1] < 0) << 1 | int(inv[2] < 0) << 2
    stack, deepest = [0], 0
    while stack:
        ref = stack.pop()
        deepest = max(deepest, len(stack))  # what a kernel holds while `ref` is its current node
        if ref < 0:
            first, cnt = (~ref) >> 3, ((~ref) & 7) + 1
            r = tri[first:first + cnt]
            t, u, v, det = _tri_eval(o, d, r[:, 0:3], r[:, 4:7], r[:, 8:11])
            with np.errstate(invalid="ignore"):
                ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)
            if ok.any():
                t_best = min(t_best, t[ok].min() * (1.0 - margin))
            continue
        hits = []
        for slot, (lo, hi, r) in enumerate(_node_slots(layout, nodes, ref)):
            pad = margin * (hi - lo)
            with np.errstate(invalid="ignore"):
                ta, tb = (lo + pad - o) * inv, (hi - pad - o) * inv
            if np.isnan(ta).any() or np.isnan(tb).any():
                continue  # a zero direction component on a slab boundary: leave the child out
            tn = max(np.minimum(ta, tb).max(), 0.0)
            tf = min(np.maximum(ta, tb).min(), t_best)
            if tn <= tf:
                hits.append(((slot ^ octant) if layout == 73 else (tn, slot), r))
        for _, r in sorted(hits, reverse=True):  # descending key: the nearest ends on top
            stack.append(r)
    return deepest
