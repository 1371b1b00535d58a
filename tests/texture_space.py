"""The texture and UV space, stated once for tests/test_texture_space.py (no device) and tests/test_gpu_texture_space.py: the sizes,
filters, texel contents and UV families docs/SPEC.md §13's domain promises, the probe scene that brings them before a camera, and the
judgement of looked-up texels against the float64 reference of tests/tex64.py. Test helpers only.

The probe scene is the jitter-free camera of env_checker.one_triangle_scene (pixel spacing 0.125 at z = -1) before a wall at z = -1 of
12 x 9 square tiles, 0.5 units wide, two triangles each: 4 x 4 pixels a tile, 216 triangles. The wall is centred on the view and turned
by 1/64 radian in its plane, so that no pixel looks at an edge or a diagonal and no two pixels of a column share a coordinate. Every
tile has a material of its own, Lambert with albedo 0.5: albedo * texel is exact. The subject is texture 1; textures 0 and 2 are guards
of 5 x 3 and 3 x 5 texels in [100, 200] bound to the four corner tiles, on both sides of the subject in the device's pool: a texel index
that leaves the subject reads a value outside the subject's envelope.

A UV family is a function from a vertex's place (a, b) in [0, 1]^2 on the wall to its (s, t); `constants` is the tile wall: the three
vertices of a tile's triangles carry the same (s0, t0), so that the f32 coordinate wanders a few ulps round s0 from pixel to pixel — the
only way a camera probe reaches fs == 1.0f, texel borders and 2^20 on the device.

Every case is near or far by its own data (tex64.near at every ideal pixel; `constants` tile by tile, each tile a case of its own),
and stated() says which it is meant to be: the module asserts at import that the two agree, and the conditions that make the space worth
probing. Pytest rewrites `assert` only in test modules, so every assert here carries its own message."""
import dataclasses

import numpy as np

import tex64
import tex_checker as tc

W, H = 48, 36
SCALE = 0.125
TX, TY, TILE = 12, 9, 0.5
THETA = 1.0 / 64.0
CENTRE = np.array([-0.0625, -0.0625])  # of the view at z = -1: pixel x looks at (x - 24) / 8, pixel y at (y - 18) / 8
ALBEDO = 0.5
SUBJECT = 1
GUARD_TILES = {0: 0, TX - 1: 2, (TY - 1) * TX: 2, TY * TX - 1: 0}  # tile -> guard texture
N_TILES, N_TRIS = TX * TY, 2 * TX * TY
MISS = 0xFFFFFFFF
FLT_MAX = float(np.finfo(np.float32).max)

# W x H. The full 4096 x 4096 is 256 MiB of float4 on the device and is left out: 4096 on each axis alone reaches the same index arithmetic.
SIZES = [(1, 1), (2, 1), (1, 2), (1, 7), (7, 1), (3, 5), (63, 65), (255, 257), (4096, 2), (2, 4096), (1024, 1024)]
FILTERS = {"bilinear": 0, "nearest": tc.NEAREST}
CONTENTS = ("distinct", "checker", "hdr", "one_colour")
FAMILIES = ("unit", "across_zero", "magnified", "minified", "mirrored", "sheared", "offset_2p10", "offset_2p16", "offset_2p20", "neg_offset_2p20",
            "constants")
SIZE_IDS = [f"{w}x{h}" for w, h in SIZES]


# ------------------------------------------------------------------------------------------------ the wall
def _rot(p, theta):
    c, s = np.cos(theta), np.sin(theta)
    return np.stack([c * p[..., 0] - s * p[..., 1], s * p[..., 0] + c * p[..., 1]], -1)


def _grid():
    """(TY + 1, TX + 1, 2) float64 world positions of the tile corners."""
    gx, gy = np.meshgrid(np.arange(TX + 1), np.arange(TY + 1))
    return CENTRE + _rot(np.stack([gx * TILE - TX * TILE / 2, gy * TILE - TY * TILE / 2], -1), THETA)


def _corners():
    """(N_TRIS, 3, 2) integer grid corners (gx, gy) of every triangle: tile n = j * TX + i has triangles 2n = (00, 10, 11) and
    2n + 1 = (00, 11, 01), counter-clockwise seen from the camera."""
    out = np.empty((N_TRIS, 3, 2), np.int64)
    for n in range(N_TILES):
        i, j = n % TX, n // TX
        out[2 * n] = [(i, j), (i + 1, j), (i + 1, j + 1)]
        out[2 * n + 1] = [(i, j), (i + 1, j + 1), (i, j + 1)]
    return out


CORNERS = _corners()


def wall_verts():
    """(N_TRIS, 9) float32."""
    g = _grid()
    xy = g[CORNERS[..., 1], CORNERS[..., 0]]
    return np.concatenate([xy, np.full(xy.shape[:2] + (1,), -1.0)], -1).reshape(N_TRIS, 9).astype(np.float32)


def sheared_verts():
    """The wall sheared in its plane (x += 0.03 y), still before the whole view but for its corners."""
    v = wall_verts().astype(np.float64).reshape(-1, 3)
    v[:, 0] += 0.03 * v[:, 1]
    return v.reshape(N_TRIS, 9).astype(np.float32)


def wall_place(xy):
    """(a, b) in [0, 1]^2 of world points (.., 2) on the unsheared wall."""
    q = _rot(np.asarray(xy, np.float64) - CENTRE, -THETA)
    return q[..., 0] / (TX * TILE) + 0.5, q[..., 1] / (TY * TILE) + 0.5


def ideal_points():
    """What the float64 camera sees: (pixel indices y * W + x that hit the wall, their triangle ids, u, v as float64)."""
    x, y = np.meshgrid((np.arange(W) - W // 2) * SCALE, (np.arange(H) - H // 2) * SCALE)
    a, b = wall_place(np.stack([x, y], -1).reshape(-1, 2))
    hit = (a >= 0) & (a < 1) & (b >= 0) & (b < 1)
    px = np.nonzero(hit)[0]
    qx, qy = a[px] * TX, b[px] * TY
    i, j = np.floor(qx).astype(np.int64), np.floor(qy).astype(np.int64)
    fx, fy = qx - i, qy - j
    first = fx > fy
    ids = 2 * (j * TX + i) + np.where(first, 0, 1)
    return px, ids, np.where(first, fx - fy, fx), np.where(first, fy, fy - fx)


IDEAL = ideal_points()


# ------------------------------------------------------------------------------------------------ the UV families
def constant_values(n):
    """The coordinates a `constants` tile may carry along an axis of n texels."""
    ks = (0, n // 2, n - 1)
    return [0.0, -0.0, 1.0, -1.0, 0.5, 1.0 - 2.0 ** -24, -2.0 ** -30, -1e-9] + [(k + 0.5) / n for k in ks] + [k / n for k in ks] + \
        [1.0 / 3.0, 2.0 ** 20, -2.0 ** 20, 2.0 ** 20 - 0.125]


def constant_pairs(size):
    """(N_TILES, 2): tile n carries value n mod 18 along s and value (7 n + n div 18) mod 18 along t — 108 different pairs in which
    every value of one axis meets six of the other."""
    ls, lt = constant_values(size[0]), constant_values(size[1])
    n = np.arange(N_TILES)
    return np.stack([np.array(ls)[n % len(ls)], np.array(lt)[(7 * n + n // len(ls)) % len(lt)]], -1)


def family_st(family, a, b, size):
    w, h = size
    if family == "unit":
        return a, b
    if family == "across_zero":
        return 3.0 * a - 1.5, 3.0 * b - 1.5
    if family == "magnified":  # the whole wall inside the cell of texel (w div 2, h div 2)
        return (w // 2 + 0.25 + 0.5 * a) / w, (h // 2 + 0.25 + 0.5 * b) / h
    if family == "minified":   # more than a repeat per pixel; S up to 64
        return 61.7 * a + 0.31, 63.9 * b - 0.17
    if family == "mirrored":   # negative determinant
        return 1.25 - 1.5 * a, 1.5 * b - 0.25
    if family == "sheared":
        return 1.25 * a + 0.5 * b - 0.3, 1.1 * b - 0.375 * a + 0.2
    shift = {"offset_2p10": 2.0 ** 10, "offset_2p16": 2.0 ** 16, "offset_2p20": 2.0 ** 20 - 1.0, "neg_offset_2p20": -2.0 ** 20}[family]
    return a + shift, b + shift  # whole repeats; [2^20 - 1, 2^20] and [-2^20, -2^20 + 1] touch SPEC §13's bound exactly


def affine(family, size):
    """The family's (s, t) = A (a, b) + c as (A (2, 2), c (2,)), from its values at three places."""
    s0, t0 = family_st(family, 0.0, 0.0, size)
    s1, t1 = family_st(family, 1.0, 0.0, size)
    s2, t2 = family_st(family, 0.0, 1.0, size)
    return np.array([[s1 - s0, s2 - s0], [t1 - t0, t2 - t0]]), np.array([s0, t0])


_uvs = {}


def uvs(size, family):
    """(N_TRIS, 6) float32."""
    key = (size if family in ("magnified", "constants") else None, family)
    if key not in _uvs:
        if family == "constants":
            st = np.repeat(constant_pairs(size), 2, axis=0)[:, None, :].repeat(3, axis=1)
        else:
            s, t = family_st(family, CORNERS[..., 0] / TX, CORNERS[..., 1] / TY, size)
            st = np.stack([s, t], -1)
        _uvs[key] = st.reshape(N_TRIS, 6).astype(np.float32)
    return _uvs[key]


# ------------------------------------------------------------------------------------------------ the textures
class Tex:
    """One texture of a probe: the H x W x 3 float32 image, its filter flags, its tex64.Stats, and what its contents allow."""

    def __init__(self, img, flags=0, hdr=False):
        self.img, self.flags, self.hdr = np.ascontiguousarray(img, np.float32), flags, hdr
        self.stats = tex64.Stats(self.img)
        self.one_colour = bool((self.stats.lo == self.stats.hi).all())
        self.size = (self.img.shape[1], self.img.shape[0])

    def with_flags(self, flags):
        t = Tex.__new__(Tex)
        t.__dict__.update(self.__dict__)
        t.flags = flags
        return t


_subjects = {}


def contents_image(size, contents):
    w, h = size
    if contents == "distinct":
        return tc.distinct(w, h)
    if contents == "checker":  # 0 / 1: the largest Dx and Dy a range of 1 allows
        x, y = np.meshgrid(np.arange(w), np.arange(h))
        return np.repeat(((x + y) & 1).astype(np.float32)[..., None], 3, axis=2)
    if contents == "hdr":      # 1e-30 .. 1e30, the last texel 0 and the first FLT_MAX
        img = (10.0 ** np.random.default_rng(w * 4099 + h).uniform(-30.0, 30.0, (h, w, 3))).astype(np.float32)
        img.reshape(-1, 3)[-1] = 0.0
        img.reshape(-1, 3)[0] = FLT_MAX
        return img
    return np.full((h, w, 3), (0.3, 0.7, 1.9), np.float32)


def subject(size, contents, flags=0):
    if (size, contents) not in _subjects:
        _subjects[(size, contents)] = Tex(contents_image(size, contents), 0, hdr=contents == "hdr")
    return _subjects[(size, contents)].with_flags(flags)


def guard(index):
    w, h = {0: (5, 3), 2: (3, 5)}[index]
    return Tex(100.0 + 90.0 * (tc.distinct(w, h, 7 + index) - 0.1), tc.NEAREST if index == 2 else 0)


GUARDS = {0: guard(0), 2: guard(2)}


# ------------------------------------------------------------------------------------------------ a probe: what is bound where
@dataclasses.dataclass
class Sheet:
    """The textures of one probe scene: per-triangle UVs, the texture of every tile's material (MISS: none), the textures set (bound
    or not), and the wall's vertices."""
    uvs: np.ndarray
    tile_texture: np.ndarray
    textures: dict
    verts: np.ndarray = dataclasses.field(default_factory=wall_verts)

    def scene(self, P):
        """The SceneData: the probe camera, the wall, one Lambert material of albedo ALBEDO per tile, a sky of exactly 1."""
        import env_checker as ec
        base = ec.one_triangle_scene(P, W, H)
        mats = np.zeros(N_TILES, base.mats.dtype)
        mats["kind"], mats["albedo"], mats["ior"] = 0, ALBEDO, 1.0
        sd = dataclasses.replace(base, verts=self.verts, tri_mat=np.repeat(np.arange(N_TILES, dtype=np.uint32), 2), mats=mats,
                                 sky=np.ones(3, np.float32))
        return dataclasses.replace(sd, uvs=self.uvs, textures={i: (t.img, t.flags) for i, t in self.textures.items()},
                                   material_textures=self.tile_texture.astype(np.uint32))


def probe(size, contents, family, flags):
    """The Sheet of one case: the subject on every tile but the corners, the guards there."""
    tt = np.full(N_TILES, SUBJECT, np.int64)
    for tile, g in GUARD_TILES.items():
        tt[tile] = g
    return Sheet(uvs(size, family), tt, {0: GUARDS[0], SUBJECT: subject(size, contents, flags), 2: GUARDS[2]})


CONTACT_BOUND = [i for i in range(64) if i % 8 not in (0, 3, 7)]  # 40 of 64: unbound textures below, between and above the bound ones


def contact_texture(i, size=None, flags=None):
    """Texture i of the contact sheet: (1 + i) x (1 + 37 i mod 64) texels unless `size` says otherwise, every texel in [i, i + 0.3) so
    that no two textures share a value and a wrong first-texel offset shows, the filters alternating."""
    w, h = (1 + i, 1 + (37 * i) % 64) if size is None else size
    return Tex(i + 0.25 * tc.distinct(w, h, i), (tc.NEAREST if i % 2 else 0) if flags is None else flags)


def contact_sheet():
    """The tile wall with all 64 textures set, 40 of them bound: tile n's material to CONTACT_BOUND[n mod 40]. Every tile spans a
    little more than one repeat along both axes, across zero."""
    s, t = CORNERS[..., 0] / TX, CORNERS[..., 1] / TY
    st = np.stack([13.0 * s + 2.0 * t - 0.4, 10.0 * t - s - 0.3], -1).reshape(N_TRIS, 6).astype(np.float32)
    return Sheet(st, np.array(CONTACT_BOUND)[np.arange(N_TILES) % len(CONTACT_BOUND)], {i: contact_texture(i) for i in range(64)})


def hold(sheet, ids, u, v, got, ctx, extra=None, only=None, st=None):
    """The texels `got` (n, 3) float32 that an f32 implementation looked up at barycentrics (u, v) of triangles `ids`, against tex64
    with every triangle's own texture: finite; inside the envelope; a one-colour texture's colour exactly; a nearest lookup one of
    tex64's candidates bit for bit; a bilinear lookup within tol at every near point of a texture that is not HDR. only: the texture
    index to judge. st: the reference's coordinates (s, t) where they are not tex64.coordinate's of (u, v), and extra (n,) what they
    may be off by in UV units: tol grows by extra (W Dx + H Dy). Returns {texture: (largest err / tol over near points or 0, near
    points, points)}."""
    ids, got = np.asarray(ids, np.int64), np.asarray(got, np.float32)
    tex_of = sheet.tile_texture[ids // 2]
    out = {}
    for k in np.unique(tex_of):
        if k == MISS or (only is not None and k != only):
            continue
        T, sel = sheet.textures[int(k)], np.nonzero(tex_of == k)[0]
        q, g = sheet.uvs[ids[sel]], got[sel]
        s, t = tex64.coordinate(q, u[sel], v[sel]) if st is None else (st[0][sel], st[1][sel])
        tol, dx, dy = tex64.bound(T.stats, q)
        assert np.isfinite(g).all(), (ctx, int(k), "not finite", sel[~np.isfinite(g).all(1)][:4].tolist())
        env = tex64.envelope(T.stats, g)
        assert env.all(), (ctx, int(k), "outside the texture's envelope", int((~env).sum()), sel[~env][:4].tolist(), g[~env][:2].tolist())
        worst, n_near = 0.0, 0
        if T.one_colour:
            assert (g == T.img[0, 0]).all(), (ctx, int(k), "a one-colour texture's colour changed", g[(g != T.img[0, 0]).any(1)][:2].tolist())
        if T.flags & tc.NEAREST:
            cand = tex64.nearest_candidates(T.img, s, t, dx, dy)
            ok = cand.holds(T.img, g)
            assert ok.all(), (ctx, int(k), "not a candidate texel", int((~ok).sum()), sel[~ok][:4].tolist(), g[~ok][:2].tolist(),
                              s[~ok][:2].tolist(), t[~ok][:2].tolist())
        elif not T.hdr:
            if extra is not None:
                tol = tol + extra[sel] * (T.size[0] * T.stats.Dx + T.size[1] * T.stats.Dy)
            nr = tex64.near(T.stats, tol)
            err = np.abs(g.astype(np.float64) - tex64.bilinear(T.img, s, t)).max(1)
            bad = nr & (err > tol)
            assert not bad.any(), (ctx, int(k), "beyond the bound", int(bad.sum()), sel[bad][:4].tolist(), (err[bad] / tol[bad]).max(),
                                   s[bad][:2].tolist(), t[bad][:2].tolist())
            n_near = int(nr.sum())
            worst = float((err[nr] / np.where(tol[nr] > 0, tol[nr], 1.0)).max()) if n_near else 0.0  # (tol = 0: an all-zero texture)
        out[int(k)] = (worst, n_near, len(sel))
    return out


def checker_texels(sheet, ids, u, v):
    """(n, 3) float32: the scalar checker's lookup(coordinate(..)) at the same points, every triangle with its tile's texture."""
    ids = np.asarray(ids, np.int64)
    tex_of = sheet.tile_texture[ids // 2]
    out = np.ones((len(ids), 3), np.float32)
    for k in np.unique(tex_of):
        if k != MISS:
            sel = np.nonzero(tex_of == k)[0]
            T = sheet.textures[int(k)]
            out[sel] = tc.lookup_many(T.img, sheet.uvs[ids[sel]], u[sel], v[sel], T.flags)[0]
    return out


# ------------------------------------------------------------------------------------------------ near and far
def stated(size, contents, family):
    """What a case is meant to be: "exact" (one colour: the colour itself), "far" (only the envelope holds: tol is past a sixteenth
    of the texel range) or "near". With Dx = Dy = range, as `distinct` and `checker` nearly have, tol <= range / 16 is
    (W + H) (6 e S + 2^-25 + e) <= 1 / 16: (W + H) S below about 170 000, or W + H below about 700 000 however small S is."""
    w, h = size
    if contents == "one_colour" or w * h == 1:
        return "exact"
    if contents == "hdr":
        return "far"      # envelope and finiteness only, whatever tol says
    if family in ("offset_2p16", "offset_2p20", "neg_offset_2p20"):
        return "far"      # (W + H) S >= 3 * 2^16
    if family == "offset_2p10":
        return "far" if w + h > 160 else "near"
    if family == "minified":
        return "far" if max(w, h) > 1000 else "near"  # 4096 + 2 at S = 64 by tol; 1024 x 1024 stated far: see the conditions
    return "near"


# Stated far although tol alone would call them near: too many of their pixels lie within a coordinate rounding of a texel border for
# the nearest filter's condition below to be asked of them (93.5 %, 91.7 % and 89.1 % of their pixels have a single candidate).
# Nothing is asserted less for it: hold() holds every near point of every case to tol, whatever the case is called.
FAR_THOUGH_NEAR_BY_TOL = {("minified", (1024, 1024)), ("offset_2p16", (2, 1)), ("offset_2p16", (1, 2))}


def data_says(size, contents, family):
    """near / far / exact from tex64 alone, over the ideal pixels of the subject's tiles (for `constants`: the (near, far) tile counts)."""
    T = subject(size, contents)
    if T.one_colour:
        return "exact"
    px, ids, u, v = IDEAL
    sub = probe(size, contents, family, 0).tile_texture[ids // 2] == SUBJECT
    tol = tex64.bound(T.stats, uvs(size, family)[ids[sub]])[0]
    nr = tex64.near(T.stats, tol)
    if family == "constants":
        tiles = ids[sub] // 2
        near_tiles = {int(n) for n in np.unique(tiles) if nr[tiles == n].all()}
        return len(near_tiles), len(np.unique(tiles)) - len(near_tiles)
    return "near" if nr.all() else "far"


def _conditions():
    px, ids, u, v = IDEAL
    assert len(px) >= 0.95 * W * H, f"only {len(px)} of {W * H} pixels hit the wall"
    for size in SIZES:
        for family in FAMILIES:
            q = uvs(size, family)[ids]
            assert np.isfinite(q).all() and np.abs(q).max() <= 2.0 ** 20, f"{family} {size}: a UV outside SPEC §13's domain"
            s, t = tex64.coordinate(q, u, v)
            for contents in ("distinct", "checker"):
                says, meant = data_says(size, contents, family), stated(size, contents, family)
                if family == "constants":
                    if meant != "exact":  # 2^20 and its kin are far on any texture of more than one texel; the rest must be near
                        assert says[0] >= 0.6 * N_TILES and says[1] >= 1, f"constants {size} {contents}: {says} near / far tiles"
                elif (family, size) in FAR_THOUGH_NEAR_BY_TOL:
                    assert (says, meant) == ("near", "far"), f"{family} {size} {contents}: listed as stated far though near by tol, but is {says}, {meant}"
                else:
                    assert says == meant, f"{family} {size} {contents}: meant {meant}, its data says {says}"
            if size == (1, 1):
                continue
            T = subject(size, "distinct")
            tol, dx, dy = tex64.bound(T.stats, q)
            cand = tex64.nearest_candidates(T.img, s, t, dx, dy)
            if family not in ("magnified", "constants"):
                x0, x1, _ = tex64._axis(s, size[0])
                y0, y1, _ = tex64._axis(t, size[1])
                seen = len(np.unique(np.concatenate([y0 * size[0] + x0, y0 * size[0] + x1, y1 * size[0] + x0, y1 * size[0] + x1])))
                assert seen >= min(size[0] * size[1], 200), f"{family} {size}: the reference sees only {seen} texels"
            if family != "constants" and stated(size, "distinct", family) == "near":
                single = float((cand.count == 1).mean())
                assert single >= 0.9, f"{family} {size}: only {100 * single:.1f} % of the pixels have a single candidate texel"


_conditions()
