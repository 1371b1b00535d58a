/*
 * denoise_ref.c — TEST INFRASTRUCTURE ONLY: a scalar restatement of docs/SPEC.md §8 (pt_denoise), written from the spec and independently
 * of pathtracing_amd/. The guide ray's closest hit and the camera ray come from the oracle (oracle/pt_oracle.h); the front-facing
 * normal, the albedo lookup, the edge-stop function and the à-trous passes are written here. Nothing in the product may include, link or
 * call this.
 *
 * dr_guides() is §8.1 on the scene's own arrays (original order), dr_filter() is §8.2 on any colour image and guide buffers, so that the
 * tests can also feed it synthetic guides. dr_pass() is one pass of §8.2, or a deliberately wrong variant of it (DRV_*): the negative
 * controls of tests/test_denoise64.py, which must fail the float64 comparison. Only the tests call it with a variant.
 */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "../../oracle/pt_oracle.h"

/* pt_denoise_params (include/ptrt.h), 32 B */
typedef struct { uint32_t iterations; float sigma_color, sigma_normal, sigma_depth, sigma_albedo; uint32_t flags; uint32_t pad[2]; } dr_params;
enum { DR_GUIDES_ONLY = 1u, DR_NO_EDGE_STOPS = 2u };

/* §8.2 defaults, as exact f32 values */
#define DR_ITERATIONS 4u
#define DR_SIGMA_COLOR 0x1p+4f   /* 16 */
#define DR_SIGMA_NORMAL 0x1p-4f  /* 0.0625 */
#define DR_SIGMA_DEPTH 0x1p-7f   /* 0.0078125 */
#define DR_SIGMA_ALBEDO 0x1p-2f  /* 0.25 */

#define MISS 0xFFFFFFFFu

static inline float fma_(float a, float b, float c) { return fmaf(a, b, c); }
static inline float dot3(const float *a, const float *b) { return fma_(a[2], b[2], fma_(a[1], b[1], a[0] * b[0])); }
static inline uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

/* §8.1: g8 = W*H*8 floats, g0 then g1 per pixel */
int dr_guides(const pto_scene *s, uint32_t W, uint32_t H, float *g8)
{
    pto_scene sc = *s;
    sc.cam.jitter = 0u; /* jx = jy = 0.5f: the key does not matter */
#pragma omp parallel for schedule(dynamic, 1)
    for (int y = 0; y < (int)H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            float o[3], d[3], t = 0.0f;
            pto_camera_ray(&sc.cam, x, (uint32_t)y, 0u, o, d);
            const uint32_t id = pto_closest(&sc, o, d, &t, NULL);
            float *g = g8 + ((size_t)y * W + x) * 8;
            if (id == MISS) {
                g[0] = g[1] = g[2] = 0.0f; g[3] = INFINITY;
                g[4] = g[5] = g[6] = 0.0f; g[7] = from_bits(MISS);
                continue;
            }
            float ng[3];
            uint32_t mat;
            if (id < sc.n_tris) { /* normalize(cross(e1, e2)) of the triangle's original vertices */
                const float *v = sc.tri_verts + (size_t)id * 9;
                const float e1[3] = { v[3] - v[0], v[4] - v[1], v[5] - v[2] }, e2[3] = { v[6] - v[0], v[7] - v[1], v[8] - v[2] };
                const float cr[3] = { fma_(e1[1], e2[2], -(e1[2] * e2[1])), fma_(e1[2], e2[0], -(e1[0] * e2[2])), fma_(e1[0], e2[1], -(e1[1] * e2[0])) };
                const float k = 1.0f / sqrtf(dot3(cr, cr));
                ng[0] = cr[0] * k; ng[1] = cr[1] * k; ng[2] = cr[2] * k;
                mat = sc.tri_mat[id];
            } else { /* (P - c) * (1.0f / r), P = madd3(t, d, o) */
                const uint32_t j = id - sc.n_tris;
                const float *c = sc.spheres + (size_t)j * 4;
                const float inv_r = 1.0f / c[3];
                const float P[3] = { fma_(t, d[0], o[0]), fma_(t, d[1], o[1]), fma_(t, d[2], o[2]) };
                ng[0] = (P[0] - c[0]) * inv_r; ng[1] = (P[1] - c[1]) * inv_r; ng[2] = (P[2] - c[2]) * inv_r;
                mat = sc.sph_mat[j];
            }
            const int front = dot3(ng, d) < 0.0f;
            for (int k = 0; k < 3; ++k) g[k] = front ? ng[k] : -ng[k];
            g[3] = t;
            for (int k = 0; k < 3; ++k) g[4 + k] = sc.mats[mat].albedo[k];
            g[7] = from_bits(id);
        }
    return 0;
}

static inline float D(float x) { return fma_(x, fma_(x, 0.5f, 1.0f), 1.0f); }

/* §8.2, the parameters with their defaults filled in; returns the number of passes (0: GUIDES_ONLY) or -1 for refused parameters */
int dr_resolve(const dr_params *in, dr_params *out)
{
    *out = *in;
    if (in->flags & ~(DR_GUIDES_ONLY | DR_NO_EDGE_STOPS)) return -1;
    if (in->iterations > 8u) return -1;
    const float sg[4] = { in->sigma_color, in->sigma_normal, in->sigma_depth, in->sigma_albedo };
    for (int k = 0; k < 4; ++k) if (!(sg[k] >= 0.0f) || isinf(sg[k])) return -1;
    if (!out->iterations) out->iterations = DR_ITERATIONS;
    if (out->sigma_color == 0.0f) out->sigma_color = DR_SIGMA_COLOR;
    if (out->sigma_normal == 0.0f) out->sigma_normal = DR_SIGMA_NORMAL;
    if (out->sigma_depth == 0.0f) out->sigma_depth = DR_SIGMA_DEPTH;
    if (out->sigma_albedo == 0.0f) out->sigma_albedo = DR_SIGMA_ALBEDO;
    return (in->flags & DR_GUIDES_ONLY) ? 0 : (int)out->iterations;
}

/* Wrong variants of a pass, for the negative controls only (0: §8.2 as written). */
enum { DRV_SPEC = 0, DRV_SIGMA_C_FIXED = 1, DRV_XZ_NO_STEP = 2, DRV_D_LINEAR = 3, DRV_WRONG_TAP = 4, DRV_NO_MISS_SKIP = 5 };

static inline float Dv(float x, int variant) { return variant == DRV_D_LINEAR ? 1.0f + x : D(x); }

/* §8.2's clamp of an inverse scale into [2^-149, FLT_MAX]: never 0 or +inf, so no 0 * inf */
static inline float clamp_scale(float v) { return fminf(fmaxf(v, 0x1p-149f), FLT_MAX); }

/* One pass i: src -> dst (W*H*4 floats each). */
static void pass(const float *src, const float *g8, uint32_t W, uint32_t H, const dr_params *p, uint32_t i, int variant, float *dst)
{
    static const float h_spec[5] = { 0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f }, h_wrong[5] = { 0.0625f, 0.25f, 0.375f, 0.25f, 0.125f };
    const float *h = variant == DRV_WRONG_TAP ? h_wrong : h_spec;
    const int s = 1 << i;
    const int edge = !(p->flags & DR_NO_EDGE_STOPS);
    const float ic = 1.0f / (p->sigma_color * p->sigma_color);
    const float ic_i = clamp_scale(variant == DRV_SIGMA_C_FIXED ? ic : ic * (float)(1u << (2u * i)));
    const float in_ = clamp_scale(1.0f / p->sigma_normal);
    const float ia = clamp_scale(1.0f / (p->sigma_albedo * p->sigma_albedo));
    const float sz = variant == DRV_XZ_NO_STEP ? 1.0f : (float)s;
#pragma omp parallel for schedule(static)
    for (int y = 0; y < (int)H; ++y)
        for (int x = 0; x < (int)W; ++x) {
            const size_t ip = (size_t)y * W + x;
            const float *cp = src + ip * 4, *gp = g8 + ip * 8;
            const int miss_p = bits(gp[7]) == MISS;
            const float iz = clamp_scale(1.0f / ((p->sigma_depth * gp[3]) * sz));
            float sw = 0.0f, sc[3] = { 0.0f, 0.0f, 0.0f };
            for (int dy = -2; dy <= 2; ++dy)
                for (int dx = -2; dx <= 2; ++dx) {
                    const int qx = x + dx * s, qy = y + dy * s;
                    if (qx < 0 || qy < 0 || qx >= (int)W || qy >= (int)H) continue;
                    const size_t iq = (size_t)qy * W + qx;
                    const float *cq = src + iq * 4, *gq = g8 + iq * 8;
                    const int miss_q = bits(gq[7]) == MISS;
                    if (miss_p != miss_q && variant != DRV_NO_MISS_SKIP) continue;
                    float den = 1.0f;
                    if (edge) {
                        const float dc[3] = { cp[0] - cq[0], cp[1] - cq[1], cp[2] - cq[2] };
                        const float xc = dot3(dc, dc) * ic_i;
                        float xn = 0.0f, xz = 0.0f, xa = 0.0f;
                        if (!miss_p) {
                            xn = fmaxf(0.0f, 1.0f - dot3(gp, gq)) * in_;
                            xz = fabsf(gq[3] - gp[3]) * iz;
                            const float da[3] = { gp[4] - gq[4], gp[5] - gq[5], gp[6] - gq[6] };
                            xa = dot3(da, da) * ia;
                        }
                        den = ((Dv(xc, variant) * Dv(xn, variant)) * Dv(xz, variant)) * Dv(xa, variant);
                    }
                    const float w = (h[dx + 2] * h[dy + 2]) / den;
                    sw = sw + w;
                    for (int k = 0; k < 3; ++k) sc[k] = fma_(w, cq[k], sc[k]);
                }
            const float r = 1.0f / sw;
            float *o = dst + ip * 4;
            if (r <= FLT_MAX) { o[0] = sc[0] * r; o[1] = sc[1] * r; o[2] = sc[2] * r; }
            else { o[0] = cp[0]; o[1] = cp[1]; o[2] = cp[2]; } /* every tap lost its weight, the centre's included: p is kept */
            o[3] = cp[3];
        }
}

/* §8.2 over rgba (W*H*4) with guides g8 into out (W*H*4). Returns the passes run, or -1 for refused parameters. */
int dr_filter(const float *rgba, const float *g8, uint32_t W, uint32_t H, const dr_params *params, float *out)
{
    dr_params p;
    const int n = dr_resolve(params, &p);
    if (n <= 0) return n;
    float *tmp = malloc((size_t)W * H * 4 * sizeof(float));
    if (!tmp) return -2;
    const float *src = rgba;
    for (int i = 0; i < n; ++i) {
        /* the last pass lands in out; the ones before alternate so that a pass never reads what it writes */
        float *dst = ((n - 1 - i) & 1) ? tmp : out;
        pass(src, g8, W, H, &p, (uint32_t)i, DRV_SPEC, dst);
        src = dst;
    }
    free(tmp);
    return n;
}

/* Pass i (0-based, step 2^i) of §8.2 alone, src -> dst, in variant `variant` (DRV_*). Returns 0, or -1 for refused parameters or i > 7. */
int dr_pass(const float *src, const float *g8, uint32_t W, uint32_t H, const dr_params *params, uint32_t i, int variant, float *dst)
{
    dr_params p;
    if (dr_resolve(params, &p) < 0 || i > 7u) return -1;
    pass(src, g8, W, H, &p, i, variant, dst);
    return 0;
}
