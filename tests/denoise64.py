"""docs/SPEC.md §8 (pt_denoise) in float64, written from the SPEC text and sharing no code with tests/denoise_ref/: the guide buffers of
§8.1 from the float64 ray caster, and one pass of the §8.2 filter with exact arithmetic, together with a per-pixel bound on how far an f32
implementation of the same pass may lie from it. Test helpers only.

`guides64` traces the unjittered camera rays (SPEC §3, from the oracle) with `ray_caster64.cast` and builds the front-facing normal, t,
albedo and id in float64 from the scene's f32 arrays; `guide_bounds` says how far an f32 implementation's normal and t may lie from them.

`atrous_pass64(img, guides, i, params)` is pass i (0-based, step 2^i) of §8.2 with the exact D(x) = 1 + x + x²/2, the same skips, a real
division and the defaults resolved as §8.2 resolves them. Compare it pass by pass: pass i's input is the implementation's own output after
i passes (the framebuffer for i = 0), so errors do not compound and the bound is a per-pass bound. The bound is derived from the
arithmetic, not fitted. With u = 2^-24 (unit roundoff) and η = 2^-149 (the spacing of subnormals), every f32 operation is modelled as
fl(a ∘ b) = (a ∘ b)(1 + θ) + ζ, |θ| <= u, |ζ| <= η, and the clamp of §8.2 as the 1-Lipschitz map it is:

* the inverse scales (ic_i, in, ia and the per-pixel iz) are evaluated as intervals under that model (an intermediate that rounds to
  +inf or 0 included), then clamped: Δscale;
* x_c = dot(c_p - c_q, c_p - c_q) * ic_i: 2u from the rounded differences, 3u + 3η from the three fmas, u + η from the product, and
  dot·Δic_i from the scale: Δx_c <= 6u·x_c + dot·Δic_i + 3η·ic_i + η. An f32 dot product that may overflow (the exact one within 8u of
  FLT_MAX or above) gives x_c = +inf and w = 0, so such a tap's weight is unknown: |Δw| = w. x_a likewise;
* x_n = max(0, 1 - dot(n_p, n_q)) * in: the dot product is off by 3u·Σ|n_p,k·n_q,k| + 3η absolute, and the cancellation in 1 - dot turns
  that into an absolute error of about 3u·in in x_n (about 4u·in with the roundings of the subtraction and the product), not a relative
  one: with the default in = 16 this is the largest term. The centre tap has x_c = x_z = x_a = 0 exactly, but x_n = max(0, 1 - |n_p|²)·in;
* x_z = |t_q - t_p| * iz: u from the subtraction, u from the product, Δiz from the interval;
* D is increasing, so |ln D32 - ln D| <= δ_D = max(ln D(x + Δx) - ln D(x), ln D(x) - ln D(x - Δx)) + 2u (its two fmas, all terms
  positive), evaluated per tap;
* w = h / (((D_c·D_n)·D_z)·D_a): |ln w32 - ln w| <= δ_w = Σ δ_D + 4u (three products, one division), so
  |Δw| <= min((e^δ_w - 1)·w, h) + 2^-125, the last term
  for a denominator that overflows to +inf in f32 (w = 0 where the exact weight is below h·2^-128) or a weight that lands on subnormals;
* a pass is a weighted mean, so with W = Σw the perturbed weights move it by at most Σ|Δw_q|·|c_q - out_p| / (W - Σ|Δw|), about
  2·δ_w·max|c_q - out_p|, as long as W - Σ|Δw| is surely above 2^-128. Below that the f32 1/sw may overflow, and §8.2 then keeps the
  pixel: the f32 result is the pixel or a weighted mean of the taps, and the bound is the hull of the taps, max|c_q - out_p|. The
  float64 pass keeps the pixel where its own W is below 1/FLT_MAX;
* the 25 fmas of Σ w·c, the 24 additions of Σ w, 1/sw and the final product round by at most 52u·max|c_q| + 200η.

The D product and x's beyond 2^300 are cut off in float64 (such a weight is below 2^-600 and counts as 0); the bound allows for it.
"""
import ctypes as C

import numpy as np

import ray_caster64 as rc

U = 2.0 ** -24
ETA = 2.0 ** -149
FLT_MAX = float(np.finfo(np.float32).max)
MISS = 0xFFFFFFFF
H5 = np.array([0.0625, 0.25, 0.375, 0.25, 0.0625])
# §8.2 defaults
DEFAULTS = dict(iterations=4, sigma_color=16.0, sigma_normal=1.0 / 16, sigma_depth=1.0 / 128, sigma_albedo=0.25)
X_CAP = 2.0 ** 300


# ================================================================================================================ §8.1 guides
def unjittered(cam):
    c = type(cam)()
    C.memmove(C.byref(c), C.byref(cam), C.sizeof(cam))
    c.jitter = 0
    return c


def guides64(pto, sd, w, h):
    """§8.1 in float64: a dict with the camera rays (o, d: f32 (R, 3)), the caster's result `cast`, ids (uint64, MISS for none), n (R, 3),
    t (R,), albedo (R, 3) float64, and the per-ray geometry `guide_bounds` needs. Rays are row-major over the w x h frame."""
    o, d = rc.camera_rays(pto, unjittered(sd.cam), w, h)
    verts = np.asarray(sd.verts, np.float32).reshape(-1, 9)
    spheres = np.asarray(sd.spheres, np.float32).reshape(-1, 4)
    cast = rc.cast(verts, spheres, o, d)
    ids, t = cast[0], cast[1]
    R, NT = len(o), len(verts)
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    n = np.zeros((R, 3))
    albedo = np.zeros((R, 3))
    mats = np.asarray(sd.mats)
    tri = ids < NT
    sph = (ids >= NT) & (ids != MISS)
    geo = dict(e1=np.zeros(R), e2=np.zeros(R), cr=np.ones(R), tv=np.zeros(R), det=np.ones(R), r=np.ones(R), oc=np.zeros(R),
               b=np.zeros(R), s=np.ones(R), c=np.zeros(R))
    if tri.any():
        j = ids[tri].astype(np.int64)
        v = verts[j].reshape(-1, 3, 3).astype(np.float64)
        e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
        cr = np.cross(e1, e2)
        n[tri] = cr / np.linalg.norm(cr, axis=1, keepdims=True)
        albedo[tri] = mats["albedo"][np.asarray(sd.tri_mat)[j]]
        geo["e1"][tri], geo["e2"][tri], geo["cr"][tri] = np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1), np.linalg.norm(cr, axis=1)
        geo["tv"][tri] = np.linalg.norm(o64[tri] - v[:, 0], axis=1)
        geo["det"][tri] = np.abs(np.einsum("ik,ik->i", e1, np.cross(d64[tri], e2)))
    if sph.any():
        j = (ids[sph] - NT).astype(np.int64)
        s4 = spheres[j].astype(np.float64)
        P = o64[sph] + t[sph, None] * d64[sph]
        n[sph] = (P - s4[:, :3]) / s4[:, 3:4]
        albedo[sph] = mats["albedo"][np.asarray(sd.sph_mat)[j]]
        oc = o64[sph] - s4[:, :3]
        geo["r"][sph], geo["oc"][sph], geo["c"][sph] = s4[:, 3], np.linalg.norm(oc, axis=1), np.linalg.norm(s4[:, :3], axis=1)
        b = np.einsum("ik,ik->i", oc, d64[sph])
        geo["b"][sph] = b
        geo["s"][sph] = np.sqrt(np.maximum(s4[:, 3] ** 2 - np.einsum("ik,ik->i", oc - b[:, None] * d64[sph], oc - b[:, None] * d64[sph]), 0))
    hit = tri | sph
    flip = np.einsum("ik,ik->i", n, d64) >= 0
    n[hit & flip] *= -1.0
    return dict(o=o, d=d, cast=cast, ids=ids, n=n, t=t, albedo=albedo, tri=tri, sph=sph, geo=geo, verts=verts, spheres=spheres)


def guide_bounds(g):
    """Per-ray bounds (dt, dn) on |t32 - t| and on each component of |n32 - n| for an f32 implementation of §4 and §8.1 that found the
    same primitive. Möller–Trumbore: the committed edges round by u each and the cross and dot products add a few u of
    |tv|·|e1|·|e2| (numerator) and |t|·|e1|·|e2| (determinant), all over |det|: dt <= u·(16|tv| + 12|t| + 4(|e1| + |e2|))·|e1||e2|/|det|
    + 4u·t. The normal normalize(cross(e1, e2)) moves by at most 8u·|e1||e2|/|cr| + 4u. Spheres: the discriminant fma(b, b, -cc) is off by
    Δ = 8u·(|oc|² + r² + b²), so the root moves by min(Δ/(2s), sqrt Δ) on top of 4u·(|oc| + t); the normal (P - c)·(1/r) moves by
    (dt + 2u(t + |o| + |c|))/r + 4u. The constants round every step's count of roundings up."""
    geo, t = g["geo"], np.where(np.isfinite(g["t"]), g["t"], 0.0)
    dt = np.zeros(len(t))
    dn = np.zeros(len(t))
    tri, sph = g["tri"], g["sph"]
    with np.errstate(divide="ignore", invalid="ignore"):
        k = geo["e1"] * geo["e2"] / geo["det"]
        dt_tri = U * (16 * geo["tv"] + 12 * t + 4 * (geo["e1"] + geo["e2"])) * k + 4 * U * t
        dn_tri = 8 * U * geo["e1"] * geo["e2"] / geo["cr"] + 4 * U
        delta = 8 * U * (geo["oc"] ** 2 + geo["r"] ** 2 + geo["b"] ** 2)
        ds = np.minimum(np.where(geo["s"] > 0, delta / (2 * geo["s"]), np.inf), np.sqrt(delta))
        dt_sph = ds + 4 * U * (geo["oc"] + t)
        o_norm = np.linalg.norm(g["o"].astype(np.float64), axis=1)
        dn_sph = (dt_sph + 2 * U * (t + o_norm + geo["c"])) / geo["r"] + 4 * U
    dt[tri], dn[tri] = dt_tri[tri], dn_tri[tri]
    dt[sph], dn[sph] = dt_sph[sph], dn_sph[sph]
    return dt, dn


def compare_guides(g32, g, w, h):
    """Check an implementation's (h, w, 8) f32 guides against guides64's `g`. Ids agree except in the classes ray_caster64.classify cannot
    settle (near an edge, coincident t, in the plane); on agreeing hits n and t lie within guide_bounds and the albedo is exact; misses are
    exactly (0, 0, 0, +inf), (0, 0, 0, MISS). Returns (n_agree, worst normal / bound, worst t / bound)."""
    g32 = g32.reshape(h * w, 8)
    got = g32[:, 7].view(np.uint32).astype(np.uint64)
    cls = rc.classify(g["verts"], g["spheres"], g["o"], g["d"], got, g["cast"])
    assert len(cls["wrong"]) == 0, ("ids", len(cls["wrong"]), cls["wrong"][:5].tolist(), got[cls["wrong"][:5]].tolist(),
                                    g["ids"][cls["wrong"][:5]].tolist())
    agree = cls["agree"]
    miss = agree[g["ids"][agree] == MISS]
    hit = agree[g["ids"][agree] != MISS]
    m = g32[miss]
    assert (m[:, :3] == 0).all() and np.isposinf(m[:, 3]).all() and (m[:, 4:7] == 0).all()
    dt, dn = guide_bounds(g)
    d64 = g["d"].astype(np.float64)
    n32 = g32[hit, :3].astype(np.float64)
    n64 = g["n"][hit]
    err_n = np.abs(n32 - n64).max(axis=1)
    # a ray that grazes the surface (|n·d| within the normal's bound) may take either side
    graze = np.abs(np.einsum("ik,ik->i", n64, d64[hit])) <= dn[hit] + 4 * U
    err_n = np.where(graze, np.minimum(err_n, np.abs(n32 + n64).max(axis=1)), err_n)
    err_t = np.abs(g32[hit, 3].astype(np.float64) - g["t"][hit])
    rn, rt = err_n / dn[hit], err_t / dt[hit]
    assert (rn <= 1).all(), ("normal", int(hit[np.argmax(rn)]), float(rn.max()), n32[np.argmax(rn)].tolist(), n64[np.argmax(rn)].tolist())
    assert (rt <= 1).all(), ("t", int(hit[np.argmax(rt)]), float(rt.max()), float(g32[hit[np.argmax(rt)], 3]), float(g["t"][hit[np.argmax(rt)]]))
    assert np.array_equal(g32[hit, 4:7].astype(np.float64), g["albedo"][hit])
    return len(agree), float(rn.max(initial=0)), float(rt.max(initial=0))


# ================================================================================================================ §8.2 filter
def resolve64(iterations=0, sigma_color=0.0, sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0, flags=0):
    """§8.2's parameter resolution: None for a refused set, else a dict with the defaults filled in and `edge` (PT_DENOISE_NO_EDGE_STOPS
    clear). The sigmas are the f32 values the API receives."""
    sig = [float(np.float32(s)) for s in (sigma_color, sigma_normal, sigma_depth, sigma_albedo)]
    if flags & ~3 or iterations > 8 or any(not (s >= 0) or np.isinf(s) for s in sig):
        return None
    names = ("sigma_color", "sigma_normal", "sigma_depth", "sigma_albedo")
    out = {k: (s if s != 0 else DEFAULTS[k]) for k, s in zip(names, sig)}
    out["iterations"] = iterations or DEFAULTS["iterations"]
    out["edge"] = not (flags & 2)
    return out


def _clamp(x):
    return np.clip(x, ETA, FLT_MAX)


def _inverse(num, den):
    """num / den in float64, and the interval of its f32 evaluation fl(num / fl(den)) before any clamp (den: the exact operand and the
    interval of its own rounding, see _rounded; a denominator that rounds to +inf gives 0, one that rounds to 0 gives +inf)."""
    den, den_lo, den_hi = den
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        v = num / den
        hi = np.where(den_lo > 0, num / np.maximum(den_lo, 1e-320) * (1 + U) + ETA, np.inf)
        lo = np.where(den_hi > FLT_MAX, 0.0, np.maximum(num / den_hi * (1 - U) - ETA, 0.0))
    return v, lo, hi


def _clamped(v, lo, hi, k=1.0):
    """clamp(k·v) in float64 and the largest deviation of the f32 clamp(fl(k·x)), x in [lo, hi], from it (k a power of two: the
    product is exact in f32 unless it overflows, and the clamp maps +inf to FLT_MAX)."""
    with np.errstate(over="ignore", invalid="ignore"):
        c = _clamp(k * v)
        return c, np.maximum(_clamp(k * hi) - c, c - _clamp(k * lo))


def _exact(x):
    return (x, x, x)


def _rounded(x):
    """the interval of fl(x) for an exact product x (an f32 result above FLT_MAX is +inf)"""
    return (x, np.maximum(x * (1 - U) - ETA, 0.0), np.where(x * (1 + U) + ETA > FLT_MAX, np.inf, x * (1 + U) + ETA))


def atrous_pass64(img, g8, i, prm):
    """Pass i of §8.2 on an (h, w, 4) image with (h, w, 8) guides, in float64. `prm`: a resolve64 dict. Returns (out (h, w, 4) float64,
    bound (h, w, 3)): the exact pass and the per-pixel, per-channel bound on an f32 implementation's deviation from it."""
    c = np.asarray(img, np.float32).astype(np.float64)
    g = np.asarray(g8, np.float32)
    h, w = c.shape[:2]
    s = 1 << i
    miss = g[..., 7].view(np.uint32) == MISS
    n = g[..., 0:3].astype(np.float64)
    t = g[..., 3].astype(np.float64)
    a = g[..., 4:7].astype(np.float64)
    sc_, sn, sz, sa = prm["sigma_color"], prm["sigma_normal"], prm["sigma_depth"], prm["sigma_albedo"]
    ic_i, d_ic = _clamped(*_inverse(1.0, _rounded(sc_ * sc_)), k=float(4 ** i))  # clamp((1/σ_c²)·4^i)
    inn, d_in = _clamped(*_inverse(1.0, _exact(sn)))
    ia, d_ia = _clamped(*_inverse(1.0, _rounded(sa * sa)))
    with np.errstate(invalid="ignore", over="ignore"):
        tz = np.where(miss, 1.0, t)
        iz, d_iz = _clamped(*_inverse(1.0, _rounded(sz * tz * s)))  # (σ_z·t_p)·s: the product by s is exact
    sw = np.zeros((h, w))
    sc = np.zeros((h, w, 3))
    taps = []  # (valid, |Δw|, colour) per tap, for the bound once the mean is known
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            ys, xs = np.arange(h) + dy * s, np.arange(w) + dx * s
            vy, vx = (ys >= 0) & (ys < h), (xs >= 0) & (xs < w)
            yc, xc_ = np.clip(ys, 0, h - 1), np.clip(xs, 0, w - 1)
            q = np.ix_(yc, xc_)
            valid = vy[:, None] & vx[None, :] & (miss == miss[q])
            cq = c[q]
            hw = H5[dx + 2] * H5[dy + 2]
            if not prm["edge"]:
                wt = np.full((h, w), hw)
                dw = np.zeros((h, w))
            else:
                wt, dw = _edge_weight(hw, c, cq, n, n[q], t, t[q], a, a[q], miss, ic_i, d_ic, inn, d_in, ia, d_ia, iz, d_iz)
            wt = np.where(valid, wt, 0.0)
            dw = np.where(valid, dw, 0.0)
            sw += wt
            sc += wt[..., None] * cq[..., :3]
            taps.append((valid, dw, cq[..., :3]))
    kept = sw < 1.0 / FLT_MAX  # 1/sw overflows: §8.2 keeps the pixel
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.concatenate([np.where(kept[..., None], c[..., :3], sc / sw[..., None]), c[..., 3:4]], axis=2)
    num = np.zeros((h, w, 3))
    sdw = np.zeros((h, w))
    cmax = np.zeros((h, w, 3))
    hull = np.zeros((h, w, 3))
    for valid, dw, cq in taps:
        num += dw[..., None] * np.abs(cq - out[..., :3])
        sdw += dw
        cmax = np.maximum(cmax, np.where(valid[..., None], np.abs(cq), 0.0))
        hull = np.maximum(hull, np.where(valid[..., None], np.abs(cq - out[..., :3]), 0.0))
    denom = sw - sdw
    # where the f32 sum of weights is surely above 2^-128 the f32 pass is a weighted mean with perturbed weights; elsewhere it is that
    # or the pixel itself, and either lies in the hull of the taps' colours
    sure = denom * (1 - 32 * U) > 2.0 ** -127
    with np.errstate(invalid="ignore", divide="ignore"):
        weighted = np.where(sure[..., None], num / np.where(sure, denom, 1.0)[..., None], np.inf)
    bound = np.minimum(weighted, hull) + 52 * U * cmax + 200 * ETA
    return out, bound


def _edge_weight(hw, cp, cq, n_p, n_q, t_p, t_q, a_p, a_q, miss, ic_i, d_ic, inn, d_in, ia, d_ia, iz, d_iz):
    """The weight of one tap in float64 and the bound on its f32 deviation |Δw| (see the module docstring)."""
    with np.errstate(over="ignore", invalid="ignore"):
        dc = cp[..., :3] - cq[..., :3]
        dot_c = (dc * dc).sum(-1)
        x_c = np.minimum(dot_c * ic_i, X_CAP)
        dx_c = 6 * U * x_c + dot_c * d_ic + 3 * ETA * ic_i + ETA
        da = a_p - a_q
        dot_a = (da * da).sum(-1)
        x_a = np.minimum(dot_a * ia, X_CAP)
        dx_a = 6 * U * x_a + dot_a * d_ia + 3 * ETA * ia + ETA
        # an f32 dot product of differences may overflow to +inf (x = +inf, w = 0) where the exact one is near or above FLT_MAX
        overflow = (dot_c * (1 + 8 * U) >= FLT_MAX) | (dot_a * (1 + 8 * U) >= FLT_MAX)
        dot = (n_p * n_q).sum(-1)
        x_n = np.maximum(0.0, 1.0 - dot) * inn
        ddot = 3 * U * np.abs(n_p * n_q).sum(-1) + 3 * ETA
        dx_n = (inn + d_in) * (ddot + U * np.abs(1.0 - dot)) + np.abs(1.0 - dot) * d_in + U * x_n + ETA
        adt = np.abs(t_q - t_p)
        x_z = np.minimum(adt * iz, X_CAP)
        dx_z = 2 * U * x_z + adt * d_iz * (1 + U) + ETA
        hit = ~miss
        x_n, dx_n = np.where(hit, x_n, 0.0), np.where(hit, dx_n, 0.0)
        x_z, dx_z = np.where(hit, x_z, 0.0), np.where(hit, dx_z, 0.0)
        x_a, dx_a = np.where(hit, x_a, 0.0), np.where(hit, dx_a, 0.0)
        overflow = np.where(hit, overflow, dot_c * (1 + 8 * U) >= FLT_MAX)
        den = np.ones(x_c.shape)
        delta = np.full(x_c.shape, 4 * U)
        for x, dx in ((x_c, dx_c), (x_n, dx_n), (x_z, dx_z), (x_a, dx_a)):
            x = np.nan_to_num(x, nan=X_CAP, posinf=X_CAP)
            dx = np.nan_to_num(dx, nan=X_CAP, posinf=X_CAP)
            lnD = lambda y: np.log1p(y + 0.5 * y * y)  # noqa: E731
            den = den * (1.0 + x + 0.5 * x * x)
            delta = delta + np.maximum(lnD(np.minimum(x + dx, X_CAP)) - lnD(x), lnD(x) - lnD(np.maximum(x - dx, 0.0))) + 2 * U
        wt = hw / den
        dw = np.minimum(np.expm1(np.minimum(delta, 50.0)) * wt, hw) + 2.0 ** -125
        dw = np.where(overflow, np.maximum(dw, wt), dw)
    return wt, dw


def pass_error(got, img, g8, i, prm):
    """(worst |got - exact| / bound over the image, index of that pixel) for an f32 pass `got` of `img`; also checks that got is finite
    and that alpha is copied."""
    got = np.asarray(got, np.float32)
    assert np.isfinite(got).all(), ("non-finite pixels", int((~np.isfinite(got)).any(axis=2).sum()), got.shape)
    assert np.array_equal(got[..., 3], np.asarray(img, np.float32)[..., 3])
    out, bound = atrous_pass64(img, g8, i, prm)
    r = np.abs(got[..., :3].astype(np.float64) - out[..., :3]) / bound
    k = int(np.argmax(r))
    return float(r.reshape(-1)[k]), np.unravel_index(k, r.shape)
