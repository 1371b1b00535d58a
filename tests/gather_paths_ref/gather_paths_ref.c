/*
 * gather_paths_ref.c — TEST INFRASTRUCTURE ONLY: a scalar restatement of docs/SPEC.md §12.1 (pt_gather_paths), written from the spec and
 * independently of pathtracing_amd/. The pieces §12.1 takes over unchanged come from the oracle (oracle/pt_oracle.h): the RNG, the
 * BSDF sample and the closest hit. Written here: §12's point rule, origin and first direction, §5's loop (the normal and emission
 * lines, throughput, Russian roulette) started at the point, §11's texel lookup, and §12's lanes, butterfly, division and clamp in plain
 * loops. Nothing in the product may include, link or call this.
 *
 * gpr_gather() also reports the exact number of segments and, for the CPU tests, every sample's radiance and segment count.
 * GPR_NO_FIRST_EMISSION, GPR_NO_W and GPR_NO_RR_DIV are deliberate errors for the tests' negative controls.
 */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif
#include "../../oracle/pt_oracle.h"

enum { GPR_NO_FIRST_EMISSION = 1, GPR_NO_W = 2, GPR_NO_RR_DIV = 4 };
typedef struct {
    uint32_t samples, seed, sample_offset, point_offset; /* samples: 1..4096, already resolved (no 0) */
    float max_distance, ray_eps;
    uint32_t max_depth, rr_start;                        /* max_depth: 1..255, already resolved */
} gpr_params;

typedef struct { float x, y, z; } v3;
static inline v3 mk(float x, float y, float z) { v3 r = { x, y, z }; return r; }
static inline float fma_(float a, float b, float c) { return fmaf(a, b, c); }
static inline float dot3(v3 a, v3 b) { return fma_(a.z, b.z, fma_(a.y, b.y, a.x * b.x)); }
static inline v3 cross3(v3 a, v3 b) { return mk(fma_(a.y, b.z, -(a.z * b.y)), fma_(a.z, b.x, -(a.x * b.z)), fma_(a.x, b.y, -(a.y * b.x))); }
static inline v3 sub3(v3 a, v3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
static inline v3 madd3(float t, v3 d, v3 o) { return mk(fma_(t, d.x, o.x), fma_(t, d.y, o.y), fma_(t, d.z, o.z)); }
static inline v3 ld3(const float *p) { return mk(p[0], p[1], p[2]); }
static inline v3 norm3(v3 v) { float s = 1.0f / sqrtf(dot3(v, v)); return mk(v.x * s, v.y * s, v.z * s); }
static inline float sgn(float x) { return copysignf(1.0f, x); }
#define MAX_GROUP 64

/* §11 encode: the texel (row-major index) of direction d in an n x n map */
static uint32_t cell(float u, uint32_t n)
{
    int i = (int)floorf(fma_(u, 0.5f, 0.5f) * (float)n);
    if (i < 0) i = 0;
    if (i > (int)n - 1) i = (int)n - 1;
    return (uint32_t)i;
}
static uint32_t texel_of(v3 d, uint32_t n)
{
    const float s = (fabsf(d.x) + fabsf(d.y)) + fabsf(d.z), is = 1.0f / s, px = d.x * is, py = d.y * is;
    float u = px, v = py;
    if (d.z < 0.0f) { u = (1.0f - fabsf(py)) * sgn(px); v = (1.0f - fabsf(px)) * sgn(py); }
    return cell(v, n) * n + cell(u, n);
}

static uint32_t closest(const pto_scene *s, v3 o, v3 d, float *t)
{
    pto_stats st;
    memset(&st, 0, sizeof st);
    const float of[3] = { o.x, o.y, o.z }, df[3] = { d.x, d.y, d.z };
    return pto_closest(s, of, df, t, &st);
}

static int finite_(float x) { return (x - x) == 0.0f; }

/* One sample: §12's ray, then §5's loop from `hit = closest(o, d)` on. acc[0..2]: the lane's E sums (fma), acc[3..5]: its bent sums,
 * *cnt its count; val[3] the sample's own radiance; returns the segments traced. */
static uint32_t one_sample(const pto_scene *s, const float *env, uint32_t env_n, const gpr_params *p, uint32_t flags, v3 o, v3 nn, uint32_t key,
                           float tmax, float acc[6], uint32_t *cnt, float val[3])
{
    static const pto_material white = { PTO_LAMBERT, { 1.0f, 1.0f, 1.0f }, { 0.0f, 0.0f, 0.0f }, 0.0f, 1.0f, { 0u, 0u, 0u } };
    const float zero[3] = { 0.0f, 0.0f, 0.0f }, nnv[3] = { nn.x, nn.y, nn.z };
    float wi0[3], W0[3], side0;
    pto_bsdf_sample(&white, zero, nnv, 1, pto_u01(key, 0), pto_u01(key, 1), 0.0f, wi0, W0, &side0); /* §5's Lambert sample: its direction */
    v3 d = ld3(wi0);
    float Tp[3] = { 1.0f, 1.0f, 1.0f };
    uint32_t depth = 0, segs = 0;
    val[0] = val[1] = val[2] = 0.0f;
    for (;;) {
        float t;
        const uint32_t id = closest(s, o, d, &t);
        segs++;
        depth++;
        if (depth == 1 && !(id != PTO_MISS && t <= tmax)) { /* §12: V_k = 1, the direction counts for bent */
            acc[3] = acc[3] + d.x; acc[4] = acc[4] + d.y; acc[5] = acc[5] + d.z;
            (*cnt)++;
        }
        if (id == PTO_MISS) {
            const float *L = env ? env + (size_t)texel_of(d, env_n) * 3 : s->sky;
            for (int k = 0; k < 3; ++k) { acc[k] = fma_(Tp[k], L[k], acc[k]); val[k] = fma_(Tp[k], L[k], val[k]); }
            break;
        }
        const v3 P = madd3(t, d, o);
        v3 ng;
        uint32_t mat;
        if (id >= s->n_tris) {
            const float *sp = s->spheres + (size_t)(id - s->n_tris) * 4;
            const float ir = 1.0f / sp[3];
            ng = mk((P.x - sp[0]) * ir, (P.y - sp[1]) * ir, (P.z - sp[2]) * ir);
            mat = s->sph_mat[id - s->n_tris];
        } else {
            const float *tv = s->tri_verts + (size_t)id * 9;
            const v3 v0 = ld3(tv);
            ng = norm3(cross3(sub3(ld3(tv + 3), v0), sub3(ld3(tv + 6), v0)));
            mat = s->tri_mat[id];
        }
        const int front = dot3(ng, d) < 0.0f;
        const v3 n = front ? ng : mk(-ng.x, -ng.y, -ng.z);
        const pto_material *m = s->mats + mat;
        if ((m->emission[0] != 0.0f || m->emission[1] != 0.0f || m->emission[2] != 0.0f) && !((flags & GPR_NO_FIRST_EMISSION) && depth == 1))
            for (int k = 0; k < 3; ++k) { acc[k] = fma_(Tp[k], m->emission[k], acc[k]); val[k] = fma_(Tp[k], m->emission[k], val[k]); }
        if (depth >= p->max_depth) break;
        const uint32_t b = depth - 1;
        const float u1 = pto_u01(key, 4 + 4 * b), u2 = pto_u01(key, 5 + 4 * b), u3 = pto_u01(key, 6 + 4 * b);
        const float dv[3] = { d.x, d.y, d.z }, nv[3] = { n.x, n.y, n.z };
        float wi[3], W[3], side;
        if (!pto_bsdf_sample(m, dv, nv, front, u1, u2, u3, wi, W, &side)) break;
        if (!(flags & GPR_NO_W)) for (int k = 0; k < 3; ++k) Tp[k] = Tp[k] * W[k];
        if (!(fmaxf(Tp[0], fmaxf(Tp[1], Tp[2])) > 0.0f)) break;
        if (depth >= p->rr_start) {
            const float qrr = fminf(fmaxf(Tp[0], fmaxf(Tp[1], Tp[2])), 0.95f);
            if (!(pto_u01(key, 7 + 4 * b) < qrr)) break;
            const float iq = 1.0f / qrr;
            if (!(flags & GPR_NO_RR_DIV)) for (int k = 0; k < 3; ++k) Tp[k] = Tp[k] * iq;
        }
        o = madd3(side * p->ray_eps, n, P);
        d = ld3(wi);
    }
    return segs;
}

static void one_point(const pto_scene *s, const float *env, uint32_t env_n, const gpr_params *p, uint32_t flags, const float *rec, uint32_t index,
                      float *out, uint64_t *rays, float *sample_rad, uint32_t *sample_segs)
{
    const uint32_t K = p->samples;
    const v3 pt = ld3(rec), nv = ld3(rec + 4);
    const float n2 = dot3(nv, nv);
    memset(out, 0, 8 * sizeof(float));
    if (sample_rad) memset(sample_rad, 0, sizeof(float) * 3 * K);
    if (sample_segs) memset(sample_segs, 0, sizeof(uint32_t) * K);
    if (!(finite_(pt.x) && finite_(pt.y) && finite_(pt.z) && finite_(n2) && n2 > 0.0f)) { out[3] = -1.0f; return; } /* §12: an invalid point */
    const v3 nn = norm3(nv), o = madd3(p->ray_eps, nn, pt);
    const float tmax = p->max_distance > 0.0f ? p->max_distance : INFINITY;
    uint32_t G = 1;
    while (G < MAX_GROUP && G < K) G *= 2;
    float lane[MAX_GROUP][6];
    uint32_t cnt = 0; /* an integer: its order does not matter */
    memset(lane, 0, sizeof lane);
    for (uint32_t g = 0; g < G; ++g)
        for (uint32_t k = g; k < K; k += G) { /* lane g: its samples in increasing k, each path to its end */
            const uint32_t key = pto_path_key(p->seed, p->point_offset + index, p->sample_offset + k);
            float val[3];
            const uint32_t segs = one_sample(s, env, env_n, p, flags, o, nn, key, tmax, lane[g], &cnt, val);
            *rays += segs;
            if (sample_rad) memcpy(sample_rad + 3 * (size_t)k, val, sizeof val);
            if (sample_segs) sample_segs[k] = segs;
        }
    for (uint32_t m = G >> 1; m; m >>= 1) { /* the butterfly: every lane s_g = s_g + s_(g xor m) */
        float next[MAX_GROUP][6];
        for (uint32_t g = 0; g < G; ++g)
            for (int j = 0; j < 6; ++j) next[g][j] = lane[g][j] + lane[g ^ m][j];
        memcpy(lane, next, sizeof next);
    }
    const float fk = (float)K;
    for (int j = 0; j < 3; ++j) out[j] = fminf(fmaxf(lane[0][j] / fk, -FLT_MAX), FLT_MAX);
    out[3] = (float)cnt / fk;
    for (int j = 0; j < 3; ++j) out[4 + j] = lane[0][3 + j] / fk;
}

/* points, out: n records of 8 floats. env (may be NULL): env_n * env_n * 3 floats, row-major. sample_rad (may be NULL): n * K * 3 floats;
 * sample_segs (may be NULL): n * K counts. *rays: the segments traced by the whole call. */
int gpr_gather(const pto_scene *s, const float *env, uint32_t env_n, const gpr_params *p, uint32_t flags, int threads, const float *points,
               uint64_t n, float *out, uint64_t *rays, float *sample_rad, uint32_t *sample_segs)
{
    if (!s || !p || !points || !out || !rays || p->samples == 0 || p->samples > 4096 || p->max_depth == 0 || p->max_depth > 255 || (env && !env_n)) return -1;
#ifdef _OPENMP
    if (threads > 0) omp_set_num_threads(threads);
#else
    (void)threads;
#endif
    uint64_t total = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : total)
    for (long long i = 0; i < (long long)n; ++i) {
        uint64_t r = 0;
        one_point(s, env, env_n, p, flags, points + 8 * (size_t)i, (uint32_t)i, out + 8 * (size_t)i, &r,
                  sample_rad ? sample_rad + 3 * (size_t)i * p->samples : NULL, sample_segs ? sample_segs + (size_t)i * p->samples : NULL);
        total += r;
    }
    *rays = total;
    return 0;
}
