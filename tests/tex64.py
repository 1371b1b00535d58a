"""docs/SPEC.md §13's texture lookup in float64, written from what the section means and not from its op order, for tests only.

A texture is a continuous, repeating image: texel k of an axis of n texels has its centre at (k + 0.5) / n, row 0 is at t = 0, and
between centres the image is the bilinear interpolation of the four nearest centres, across the wrap as anywhere else; the nearest
filter returns the texel whose cell [k, k + 1) / n holds the coordinate. The coordinate of a hit is the barycentric mean of the three
vertices' coordinates. Inputs are the f32 values the product sees, widened exactly; everything here is numpy float64, vectorised over
points. Nothing is taken from tests/tex_ref/ or pathtracing_amd/.

The tolerance is derived, not measured (bound()). With e = 2^-24, S the largest |component| of the triangle's six UVs, Dx / Dy the
largest absolute difference of horizontally / vertically adjacent texels (wrap included) and M the largest texel:

    ds  = 6 e S + 2^-25              w0's two roundings, one product, two fmas; the wrap's one rounding
    dx  = W ds + W e + 2^-25         fma(fs, Wf, -0.5), xf - floorf(xf)
    dy  = H ds + H e + 2^-25
    tol = dx Dx + dy Dy + 4 e M      bilinear is Lipschitz in texel units with constants Dx, Dy; three lerps

It says nothing once W S is around 2^21 (SPEC §13: "at least 3 fraction bits"): a point is `near` when tol <= (max texel - min
texel) / 16, and only near points are held to it. Two things hold at every point, near or far: the bilinear result lies in
[min texel (1 - 4 e), max texel (1 + 4 e)], and the nearest result is one of the texture's own texels."""
import numpy as np

E = 2.0 ** -24


def coordinate(uv6, u, v):
    """(s, t) at barycentrics (u, v) of triangles with uv6 = s0, t0, s1, t1, s2, t2 (one row per point)."""
    q = np.asarray(uv6, np.float64).reshape(-1, 6)
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    w = 1.0 - u - v
    return w * q[:, 0] + u * q[:, 2] + v * q[:, 4], w * q[:, 1] + u * q[:, 3] + v * q[:, 5]


def _axis(c, n):
    x = (c - np.floor(c)) * n - 0.5
    x0 = np.floor(x)
    return x0.astype(np.int64) % n, (x0.astype(np.int64) + 1) % n, x - x0


def bilinear(img, s, t):
    """(points, 3): the repeat-wrapped bilinear interpolation of the texel centres of the H x W x 3 image at (s, t)."""
    p = np.asarray(img, np.float64)
    h, w = p.shape[:2]
    x0, x1, fx = _axis(np.asarray(s, np.float64), w)
    y0, y1, fy = _axis(np.asarray(t, np.float64), h)
    fx, fy = fx[:, None], fy[:, None]
    top = (1.0 - fx) * p[y0, x0] + fx * p[y0, x1]
    bot = (1.0 - fx) * p[y1, x0] + fx * p[y1, x1]
    return (1.0 - fy) * top + fy * bot


class Candidates:
    """Per point the texels whose cell meets [x - dx, x + dx] x [y - dy, y + dy], as inclusive unwrapped index ranges (x_lo .. x_hi,
    y_lo .. y_hi; an index k stands for texel k mod n). count: how many different texels that is."""

    def __init__(self, w, h, x_lo, x_hi, y_lo, y_hi):
        self.w, self.h, self.x_lo, self.x_hi, self.y_lo, self.y_hi = w, h, x_lo, x_hi, y_lo, y_hi
        self.nx, self.ny = np.minimum(x_hi - x_lo + 1, w), np.minimum(y_hi - y_lo + 1, h)
        self.count = self.nx * self.ny

    def texels(self, i):
        """The set of (x, y) of point i."""
        return {(int(self.x_lo[i] + a) % self.w, int(self.y_lo[i] + b) % self.h) for a in range(int(self.nx[i])) for b in range(int(self.ny[i]))}

    def holds(self, img, got, cap=1024):
        """Per point: whether got[i] is, bit for bit, one of its candidate texels. A point with more than `cap` candidates (a far
        point: the set is most of the texture) is held to the whole texture instead."""
        px = np.ascontiguousarray(img, np.float32).view(np.uint32)
        g = np.ascontiguousarray(got, np.float32).view(np.uint32)
        ok = np.zeros(len(g), bool)
        small = self.count <= cap
        idx = np.nonzero(small)[0]
        if len(idx):
            for a in range(int(self.nx[idx].max())):
                for b in range(int(self.ny[idx].max())):
                    live = idx[(a < self.nx[idx]) & (b < self.ny[idx]) & ~ok[idx]]
                    ok[live] = (px[(self.y_lo[live] + b) % self.h, (self.x_lo[live] + a) % self.w] == g[live]).all(1)
        if (~small).any():
            ok[~small] = is_texel(img, got[~small])
        return ok


def nearest_candidates(img, s, t, dx, dy):
    h, w = np.asarray(img).shape[:2]
    s, t = np.asarray(s, np.float64), np.asarray(t, np.float64)
    x, y = (s - np.floor(s)) * w, (t - np.floor(t)) * h
    lo = lambda c, d: np.floor(c - d).astype(np.int64)  # noqa: E731
    return Candidates(w, h, lo(x, dx), lo(x, -np.asarray(dx)), lo(y, dy), lo(y, -np.asarray(dy)))


def _words(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1, 3).view(np.uint32)


def _hash(w):
    """One 64-bit word per RGB row: equal rows hash alike, and that is all is_texel needs of it."""
    w = w.astype(np.uint64)
    return w[:, 0] * np.uint64(0x9E3779B97F4A7C15) + w[:, 1] * np.uint64(0xC2B2AE3D27D4EB4F) + w[:, 2] * np.uint64(0x165667B19E3779F9)


_texels = {}


def is_texel(img, got):
    """Per row of got: whether it is, bit for bit, one of the image's texels. The image's rows are looked up by hash; a row that the
    texel found there does not equal is searched for in the whole image."""
    if id(img) not in _texels:
        rows = _words(img)
        h = _hash(rows)
        order = np.argsort(h, kind="stable")
        _texels[id(img)] = (img, h[order], rows[order])  # (the image is kept so that its id stays its own)
    _, hs, rows = _texels[id(img)]
    g = _words(got)
    ok = (rows[np.minimum(np.searchsorted(hs, _hash(g)), len(hs) - 1)] == g).all(1)
    for j in np.nonzero(~ok)[0]:
        ok[j] = (rows == g[j]).all(1).any()
    return ok


class Stats:
    """What bound() and the envelope need of an H x W x 3 image: Dx, Dy, M, the range and the per-channel extremes."""

    def __init__(self, img):
        p = np.asarray(img, np.float64)
        self.h, self.w = p.shape[:2]
        self.Dx = float(np.abs(p - np.roll(p, -1, axis=1)).max())
        self.Dy = float(np.abs(p - np.roll(p, -1, axis=0)).max())
        self.M, self.range = float(p.max()), float(p.max() - p.min())
        self.lo, self.hi = p.reshape(-1, 3).min(0), p.reshape(-1, 3).max(0)


def bound(stats, uv6, W=None, H=None):
    """(tol, dx, dy) per point: the tolerance of the module docstring and the coordinate's error in texels along both axes, from the
    image's Stats and the six UVs of each point's triangle."""
    W, H = stats.w if W is None else W, stats.h if H is None else H
    S = np.abs(np.asarray(uv6, np.float64).reshape(-1, 6)).max(1)
    ds = 6.0 * E * S + 2.0 ** -25
    dx, dy = W * ds + W * E + 2.0 ** -25, H * ds + H * E + 2.0 ** -25
    return dx * stats.Dx + dy * stats.Dy + 4.0 * E * stats.M, dx, dy


def near(stats, tol):
    """Per point: whether the bound still tells a right lookup from a wrong one."""
    return tol <= stats.range / 16.0


def envelope(stats, got):
    """Per point: got within [min texel (1 - 4 e), max texel (1 + 4 e)], channel by channel."""
    g = np.asarray(got, np.float64)
    return ((g >= stats.lo * (1.0 - 4.0 * E)) & (g <= stats.hi * (1.0 + 4.0 * E))).all(1)
