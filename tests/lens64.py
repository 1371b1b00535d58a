"""docs/SPEC.md §3.1 (the thin-lens camera ray) evaluated in float64 on the f32 words the device gets, and a first-order bound on what
the f32 evaluation may differ from it by. Written from the section's text; imports nothing from tests/lens_ref/ or from the product.
Test helpers only, vectorised over rays: tests/test_lens_space.py holds the checker to it, tests/test_gpu_lens_space.py the device.

Pytest rewrites `assert` only in test modules, so every assert here carries its own message."""
import numpy as np

U = 2.0 ** -24  # the unit roundoff of float32

# |sincos2pi(u) - (sin, cos)(2 pi u)|, which SPEC §0 does not state. Measured through the checker (lr_sincos2pi_error of tests/lens_ref/:
# pto_sincos2pi against libm's double sin and cos) over every value u01 can take, all 2^24 of them: 1.4487e-07 = 2.4305 u. The bound takes
# 3 u, a margin of 1.23; tests/test_lens_space.py test_sincos2pi_error repeats the measurement and holds it to this.
SINCOS_MEASURED = 2.4305 * U
SINCOS_ERR = 3.0 * U

VARIANTS = ("aperture_dropped_from_d", "aperture_dropped_from_o")  # deliberate errors for the negative controls


def words(cam):
    """The sixteen words of any ctypes struct with the pt_camera layout: (15 float32 values, the jitter flag)."""
    raw = np.frombuffer(bytes(cam), np.uint8)
    assert raw.size == 64, ("lens64.words: a pt_camera is 64 bytes", raw.size)
    return raw[:60].view(np.float32).copy(), int(raw[60:].view(np.uint32)[0])


class Cam:
    """A camera's words in float64."""

    def __init__(self, cam):
        w, self.jitter = words(cam)
        w = w.astype(np.float64)
        self.o, self.f, self.r, self.u, (self.scale, self.cx, self.cy) = w[0:3], w[3:6], w[6:9], w[9:12], w[12:15]


def axes64(c, R):
    """The host's lens_u = R right / |right| and lens_v = R up / |up| in float64."""
    return R * c.r / np.linalg.norm(c.r), R * c.u / np.linalg.norm(c.u)


def _terms(cam, lens, x, y, draws):
    c = Cam(cam)
    R, F = (float(np.float32(v)) for v in lens)
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    jx, jy, u2, u3 = (np.asarray(draws, np.float32).astype(np.float64)[..., k] for k in range(4))
    tx, ty = (x + jx) * c.scale, (y + jy) * c.scale
    sx, sy = tx - c.cx, ty - c.cy
    v = c.f + sx[..., None] * c.r + sy[..., None] * c.u
    r = np.sqrt(u2)
    lx, ly = r * np.cos(2.0 * np.pi * u3), r * np.sin(2.0 * np.pi * u3)
    lu, lv = axes64(c, R)
    a = ly[..., None] * lv + lx[..., None] * lu
    return c, R, F, (x, y, jx, jy), (tx, ty, sx, sy), v, (r, lx, ly), (lu, lv), a


def ray64(cam, lens, x, y, draws, variant=None):
    """§3.1 in float64. cam: a pt_camera (its f32 words are widened exactly); lens = (R, F), taken as f32; x, y: pixel coordinates (arrays
    of one shape); draws: (..., 4) the f32 values (jx, jy, u2, u3) = u01(key, 0 .. 3), with jx = jy = 0.5 where the camera's jitter is off.
    sincos2pi(u3) is (sin, cos)(2 pi u3). Returns (o64, d64), each (..., 3); d64 has length 1.

    variant: one of VARIANTS — d without -a, or o without a."""
    assert variant is None or variant in VARIANTS, ("lens64.ray64: unknown variant", variant)
    c, R, F, _, _, v, _, _, a = _terms(cam, lens, x, y, draws)
    o = c.o + (0.0 if variant == "aperture_dropped_from_o" else a)
    w = F * v - (0.0 if variant == "aperture_dropped_from_d" else a)
    return o, w / np.linalg.norm(w, axis=-1, keepdims=True)


def ray_bound(cam, lens, x, y, draws):
    """First-order bounds on the f32 ray of §3.1 against ray64: (E_o (..., 3) per component of o, the angle to d64 (...)). u = 2^-24.

    The host's axes. dot(right, right) has three roundings of positive partial sums (3 u), its square root halves that and adds its own
    half ulp (2.5 u), the reciprocal, the product with R and the product with right.k add u each:

        |d lens_u.k| <= 5.5 u |lens_u.k|                                                          (likewise lens_v)

    The point on the lens. r = fl(sqrt(u2)) is off by u r (half an ulp); sn and cs by e = SINCOS_ERR each (measured, see above);
    lx = fl(r cs):

        |d lx| <= r e + 2 u |lx|                                                                  (likewise ly with sn)

    a.k = fma(ly, lens_v.k, fl(lx lens_u.k)): the inputs' errors, one rounding of the product and one of the fma:

        |d a.k| <= A_k = |lens_u.k| (|d lx| + 6.5 u |lx|) + |lens_v.k| (|d ly| + 5.5 u |ly|) + u |a.k|

    o.k = fl(origin.k + a.k): half an ulp of the sum, at most u |o.k| — under a far camera this is the whole effect of a small aperture,
    which the origin's grid absorbs while d keeps the exact -a: the ray misses the focal point by that much — plus the error of a.k:

        |d o.k| <= u |o.k| + A_k + 2^-150

    v. As test_camera_space.angle_bound derives, but x + jx is rounded too when the pixel is jittered (j = 2, else x + 0.5 is exact and
    j = 1): |d tx| <= j u |tx|, |d sx| <= u |sx| + |d tx|, and the two fmas:

        |d v.k| <= V_k = u ((3 |sx| + j |tx|) |right_k| + (2 |sy| + j |ty|) |up_k| + 2 |forward_k|)

    w.k = fma(F, v.k, -a.k): |d w.k| <= W_k = F V_k + A_k + u |w.k|. normalize multiplies every component by the same s, whose own error
    turns nothing; its three products add one rounding each, a vector of length <= u |d|. So

        angle <= |W| / |F v - a| + u,                      taken times 1 + 2^-10 for the second-order terms.

    Valid inside §3.1's domain, where dot(w, w) neither overflows nor goes subnormal."""
    c, R, F, (x, y, jx, jy), (tx, ty, sx, sy), v, (r, lx, ly), (lu, lv), a = _terms(cam, lens, x, y, draws)
    e = SINCOS_ERR
    dlx, dly = r * e + 2 * U * np.abs(lx), r * e + 2 * U * np.abs(ly)
    A = (np.abs(lu) * (dlx + 6.5 * U * np.abs(lx))[..., None] + np.abs(lv) * (dly + 5.5 * U * np.abs(ly))[..., None] + U * np.abs(a))
    E_o = U * np.abs(c.o + a) + A + 2.0 ** -150
    exact = lambda p, j: (np.float32(p) + np.float32(j)).astype(np.float64) == p + j  # noqa: E731
    kx, ky = np.where(exact(x, jx), 1.0, 2.0), np.where(exact(y, jy), 1.0, 2.0)
    V = U * ((3 * np.abs(sx) + kx * np.abs(tx))[..., None] * np.abs(c.r) + (2 * np.abs(sy) + ky * np.abs(ty))[..., None] * np.abs(c.u)
             + 2 * np.abs(c.f))
    w = F * v - a
    Wk = F * V + A + U * np.abs(w)
    angle = (np.linalg.norm(Wk, axis=-1) / np.linalg.norm(w, axis=-1) + U) * (1 + 2.0 ** -10)
    return E_o, angle


def angle_to(d, d64):
    """The angle between the f32 directions d and the float64 directions d64."""
    d = np.asarray(d, np.float32).astype(np.float64)
    return np.arctan2(np.linalg.norm(np.cross(d, d64), axis=-1), (d * d64).sum(-1))
