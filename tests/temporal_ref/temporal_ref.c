/*
 * temporal_ref.c — TEST INFRASTRUCTURE ONLY: a scalar restatement of docs/SPEC.md §9 (pt_denoise_temporal), written from the spec and
 * independently of pathtracing_amd/. The camera rays come from the oracle (oracle/pt_oracle.h pto_camera_ray), the guides from
 * tests/denoise_ref/ (§8.1); the reprojection, the tap tests and the blend are written here. Nothing in the product may include, link or
 * call this.
 *
 * The history is the caller's: tr_accumulate() takes the frame, this call's guides and camera, the previous call's guides, accumulated
 * colour with lengths and camera (or none), and returns the accumulated image, the new history plane and, on request, where every pixel
 * was reprojected to. `variant` selects §9 as written or a deliberately wrong version of it (TRV_*): the negative controls of
 * tests/test_temporal.py. Only the tests call it with a variant.
 */
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "../../oracle/pt_oracle.h"

/* pt_temporal_params (include/ptrt.h), 32 B */
typedef struct { uint32_t max_history; float plane_tolerance, normal_min; uint32_t flags; uint32_t pad[4]; } tr_params;
enum { TR_RESET = 1u, TR_MATCH_IDS = 2u };

/* §9 defaults, as exact f32 values */
#define TR_MAX_HISTORY 32u
#define TR_MAX_HISTORY_LIMIT 1048576u
#define TR_TAU_P 0x1p-7f
#define TR_TAU_N 0.875f

#define MISS 0xFFFFFFFFu

/* Wrong variants, for the negative controls only (0: §9 as written): cam used for cam'; no plane test; the nearest old pixel with weight 1
 * instead of the four bilinear taps; a = 1/max_history whatever the length. */
enum { TRV_SPEC = 0, TRV_NO_REPROJECTION = 1, TRV_NO_PLANE_TEST = 2, TRV_NEAREST_TAP = 3, TRV_FIXED_ALPHA = 4 };

static inline float fma_(float a, float b, float c) { return fmaf(a, b, c); }
static inline float dot3(const float *a, const float *b) { return fma_(a[2], b[2], fma_(a[1], b[1], a[0] * b[0])); }
static inline void cross3(const float *a, const float *b, float *o)
{
    o[0] = fma_(a[1], b[2], -(a[2] * b[1])); o[1] = fma_(a[2], b[0], -(a[0] * b[2])); o[2] = fma_(a[0], b[1], -(a[1] * b[0]));
}
static inline uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

/* the parameters with their defaults filled in; 0, or -1 for refused parameters */
int tr_resolve(const tr_params *in, tr_params *out)
{
    *out = *in;
    if (in->flags & ~(TR_RESET | TR_MATCH_IDS)) return -1;
    if (in->max_history > TR_MAX_HISTORY_LIMIT) return -1;
    if (!(in->plane_tolerance >= 0.0f) || isinf(in->plane_tolerance)) return -1;
    if (!(in->normal_min >= 0.0f && in->normal_min <= 1.0f)) return -1;
    if (!out->max_history) out->max_history = TR_MAX_HISTORY;
    if (out->plane_tolerance == 0.0f) out->plane_tolerance = TR_TAU_P;
    if (out->normal_min == 0.0f) out->normal_min = TR_TAU_N;
    return 0;
}

typedef struct { float sw, sc[3], sl; } sums;

/* one tap of §9: old pixel (qx, qy) with weight bw */
static void tap(int qx, int qy, float bw, uint32_t W, uint32_t H, const float *old_g8, const float *old_h, const pto_camera *oc,
                const float *P, const float *n, uint32_t id, float e2, float tp2, float tau_n, int match, int variant, sums *s)
{
    if (qx < 0 || qy < 0 || qx >= (int)W || qy >= (int)H) return;
    const size_t iq = (size_t)qy * W + (size_t)qx;
    const float *gq = old_g8 + iq * 8, *hq = old_h + iq * 4;
    if (bits(gq[7]) == MISS) return;
    float o2[3], d2[3];
    pto_camera_ray(oc, (uint32_t)qx, (uint32_t)qy, 0u, o2, d2); /* oc->jitter == 0 */
    const float P2[3] = { fma_(gq[3], d2[0], o2[0]), fma_(gq[3], d2[1], o2[1]), fma_(gq[3], d2[2], o2[2]) };
    const float dP[3] = { P2[0] - P[0], P2[1] - P[1], P2[2] - P[2] };
    const float k = dot3(dP, n);
    if (variant != TRV_NO_PLANE_TEST && !(k * k <= tp2 * e2)) return;
    if (!(dot3(n, gq) >= tau_n)) return;
    if (match && bits(gq[7]) != id) return;
    s->sw = s->sw + bw;
    for (int c = 0; c < 3; ++c) s->sc[c] = fma_(bw, hq[c], s->sc[c]);
    s->sl = fma_(bw, hq[3], s->sl);
}

/*
 * §9 for one call. frame: W*H*4; g8: W*H*8 (§8.1 of this call); cam: the scene's camera. History: old_g8, old_h (W*H*4: accumulated rgb |
 * length) and old_cam of the previous call, of the same size — old_cam == NULL: no history (the caller passes none after a size change;
 * TR_RESET and max_history == 1 are handled here). out: W*H*4 accumulated rgb | frame alpha; new_h: W*H*4 accumulated rgb | length;
 * reproj (may be NULL): W*H*3 = (fx, fy, valid), valid = 1 where a hit pixel's position projects into the old image's tap range
 * (the pixel's own coordinates under an unchanged camera), else 0. Returns the number of pixels with l > 1, or -1 for refused parameters.
 */
long tr_accumulate(const float *frame, const float *g8, const pto_camera *cam, uint32_t W, uint32_t H, const float *old_g8,
                   const float *old_h, const pto_camera *old_cam, const tr_params *params, int variant, float *out, float *new_h,
                   float *reproj)
{
    tr_params p;
    if (tr_resolve(params, &p) < 0) return -1;
    const int history = old_cam && old_g8 && old_h && !(p.flags & TR_RESET) && p.max_history != 1u;
    pto_camera c0 = *cam, c1 = history ? (variant == TRV_NO_REPROJECTION ? *cam : *old_cam) : *cam;
    const int same = memcmp(&c0, &c1, sizeof c0) == 0; /* the 16 words, jitter included */
    c0.jitter = 0u; c1.jitter = 0u;
    const float tp2 = p.plane_tolerance * p.plane_tolerance, maxl = (float)p.max_history;
    const int match = (p.flags & TR_MATCH_IDS) != 0;
    float A[3], B[3], Cx[3];
    cross3(c1.right, c1.up, A); cross3(c1.up, c1.forward, B); cross3(c1.forward, c1.right, Cx);
    const float det = dot3(c1.forward, A);
    long taken = 0;
#pragma omp parallel for schedule(static) reduction(+ : taken)
    for (int y = 0; y < (int)H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            const size_t ip = (size_t)y * W + x;
            const float *c = frame + ip * 4, *g = g8 + ip * 8;
            float *o = out + ip * 4, *nh = new_h + ip * 4;
            float l = 1.0f;
            o[0] = c[0]; o[1] = c[1]; o[2] = c[2]; o[3] = c[3];
            if (reproj) { reproj[ip * 3] = reproj[ip * 3 + 1] = reproj[ip * 3 + 2] = 0.0f; }
            const uint32_t id = bits(g[7]);
            if (history && id != MISS) {
                float ro[3], rd[3];
                pto_camera_ray(&c0, x, (uint32_t)y, 0u, ro, rd);
                const float P[3] = { fma_(g[3], rd[0], ro[0]), fma_(g[3], rd[1], ro[1]), fma_(g[3], rd[2], ro[2]) };
                const float wv[3] = { P[0] - c1.origin[0], P[1] - c1.origin[1], P[2] - c1.origin[2] };
                const float e2 = dot3(wv, wv);
                sums s = { 0.0f, { 0.0f, 0.0f, 0.0f }, 0.0f };
                if (same) {
                    if (reproj) { reproj[ip * 3] = (float)x; reproj[ip * 3 + 1] = (float)y; reproj[ip * 3 + 2] = 1.0f; }
                    tap((int)x, y, 1.0f, W, H, old_g8, old_h, &c1, P, g, id, e2, tp2, p.normal_min, match, variant, &s);
                } else {
                    const float den = dot3(wv, A);
                    if ((den > 0.0f && det > 0.0f) || (den < 0.0f && det < 0.0f)) {
                        const float inv = 1.0f / den;
                        const float sx = dot3(wv, B) * inv, sy = dot3(wv, Cx) * inv;
                        const float fx = (sx + c1.cx) / c1.scale - 0.5f, fy = (sy + c1.cy) / c1.scale - 0.5f;
                        if (fx >= -1.0f && fx < (float)W && fy >= -1.0f && fy < (float)H) {
                            if (reproj) { reproj[ip * 3] = fx; reproj[ip * 3 + 1] = fy; reproj[ip * 3 + 2] = 1.0f; }
                            if (variant == TRV_NEAREST_TAP) {
                                tap((int)floorf(fx + 0.5f), (int)floorf(fy + 0.5f), 1.0f, W, H, old_g8, old_h, &c1, P, g, id, e2, tp2,
                                    p.normal_min, match, variant, &s);
                            } else {
                                const float x0 = floorf(fx), y0 = floorf(fy), bx = fx - x0, by = fy - y0;
                                for (int j = 0; j < 2; ++j)
                                    for (int i = 0; i < 2; ++i)
                                        tap((int)x0 + i, (int)y0 + j, (i ? bx : 1.0f - bx) * (j ? by : 1.0f - by), W, H, old_g8, old_h, &c1,
                                            P, g, id, e2, tp2, p.normal_min, match, variant, &s);
                            }
                        }
                    }
                }
                if (s.sw >= 0.25f) {
                    const float r = 1.0f / s.sw;
                    l = fminf(s.sl * r + 1.0f, maxl);
                    const float a = variant == TRV_FIXED_ALPHA ? 1.0f / maxl : 1.0f / l;
                    for (int k = 0; k < 3; ++k) { const float hk = s.sc[k] * r; o[k] = fma_(a, c[k] - hk, hk); }
                }
            }
            nh[0] = o[0]; nh[1] = o[1]; nh[2] = o[2]; nh[3] = l;
            taken += l > 1.0f;
        }
    return taken;
}
