/*
 * nee_ref.c — TEST INFRASTRUCTURE ONLY: a scalar restatement of docs/SPEC.md §7 (next-event estimation), written from the spec and
 * independently of pathtracing_amd/. The pieces §7 takes over unchanged come from the oracle (oracle/pt_oracle.h): the closest hit,
 * the BSDF sample, the camera ray and the RNG. The light table, the light sample, the shadow ray, the MIS weights and the
 * accumulation are written here. Nothing in the product may include, link or call this.
 *
 * nr_render() with flags = 0 is §5 (it must equal pto_render bit for bit); with NR_NEE it is §7. It also reports the extension and
 * shadow rays separately and, optionally, per-pixel sums of squared per-sample radiance (for variance estimates). NR_NO_MIS,
 * NR_NO_COSL and NR_SWAP_PMF are deliberate errors for the tests' negative controls.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif
#include "../../oracle/pt_oracle.h"

enum { NR_NEE = 1, NR_NO_MIS = 2, NR_NO_COSL = 4, NR_SWAP_PMF = 8 };
typedef struct { uint64_t ext_rays, shadow_rays, paths, n_lights; } nr_stats;

typedef struct { float x, y, z; } v3;
static inline v3 mk(float x, float y, float z) { v3 r = { x, y, z }; return r; }
static inline float fma_(float a, float b, float c) { return fmaf(a, b, c); }
static inline float dot3(v3 a, v3 b) { return fma_(a.z, b.z, fma_(a.y, b.y, a.x * b.x)); }
static inline v3 cross3(v3 a, v3 b) { return mk(fma_(a.y, b.z, -(a.z * b.y)), fma_(a.z, b.x, -(a.x * b.z)), fma_(a.x, b.y, -(a.y * b.x))); }
static inline v3 sub3(v3 a, v3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
static inline v3 madd3(float t, v3 d, v3 o) { return mk(fma_(t, d.x, o.x), fma_(t, d.y, o.y), fma_(t, d.z, o.z)); }
static inline v3 ld3(const float *p) { return mk(p[0], p[1], p[2]); }
static inline v3 norm3(v3 v) { float s = 1.0f / sqrtf(dot3(v, v)); return mk(v.x * s, v.y * s, v.z * s); }
static inline float comp(v3 v, int k) { return k == 0 ? v.x : k == 1 ? v.y : v.z; }
static inline float nan0(float w) { return w >= 0.0f ? w : 0.0f; }
#define INV_PI 0.318309873f
#define MAX_STREAMS 64

typedef struct { v3 v0, e1, e2, nl; float area, pmf, pa; const float *le; } light_t;
typedef struct {
    uint32_t n; light_t *l; float *cdf;
    float *pa_of; /* per original triangle id: pa of the light it is, else 0 */
} table_t;

/* §7 light set: triangles whose material emits, with area > 0 and w = area * (e.r + e.g + e.b) > 0 (in double), in triangle order */
static int build_table(const pto_scene *s, uint32_t flags, table_t *T)
{
    memset(T, 0, sizeof *T);
    T->l = calloc(s->n_tris ? s->n_tris : 1, sizeof(light_t));
    T->cdf = calloc(s->n_tris ? s->n_tris : 1, sizeof(float));
    T->pa_of = calloc(s->n_tris ? s->n_tris : 1, sizeof(float));
    double *w = calloc(s->n_tris ? s->n_tris : 1, sizeof(double)), total = 0.0;
    uint32_t *id = calloc(s->n_tris ? s->n_tris : 1, sizeof(uint32_t));
    if (!T->l || !T->cdf || !T->pa_of || !w || !id) return -1;
    for (uint32_t i = 0; i < s->n_tris; ++i) {
        const float *e = s->mats[s->tri_mat[i]].emission;
        if (e[0] == 0.0f && e[1] == 0.0f && e[2] == 0.0f) continue;
        const float *p = s->tri_verts + (size_t)i * 9;
        light_t L;
        L.v0 = ld3(p); L.e1 = sub3(ld3(p + 3), L.v0); L.e2 = sub3(ld3(p + 6), L.v0);
        const v3 cr = cross3(L.e1, L.e2);
        L.area = 0.5f * sqrtf(dot3(cr, cr));
        const double wi = (double)L.area * ((double)e[0] + (double)e[1] + (double)e[2]);
        if (!(L.area > 0.0f) || !(wi > 0.0)) continue;
        L.nl = norm3(cr); L.le = e;
        w[T->n] = wi; id[T->n] = i; T->l[T->n++] = L;
        total += wi;
    }
    double run = 0.0;
    for (uint32_t j = 0; j < T->n; ++j) {
        run += w[j];
        T->cdf[j] = j + 1 == T->n ? 1.0f : (float)(run / total);
        T->l[j].pmf = (float)(w[j] / total);
    }
    if ((flags & NR_SWAP_PMF) && T->n >= 2) { float t = T->l[0].pmf; T->l[0].pmf = T->l[1].pmf; T->l[1].pmf = t; }
    for (uint32_t j = 0; j < T->n; ++j) { T->l[j].pa = T->l[j].pmf / T->l[j].area; T->pa_of[id[j]] = T->l[j].pa; }
    free(w); free(id);
    return 0;
}

static uint32_t pick(const table_t *T, float u)
{
    uint32_t i = 0;
    while (!(u < T->cdf[i])) ++i; /* the smallest i with u < cdf[i]; cdf[n - 1] = 1 > u */
    return i;
}

static uint32_t closest(const pto_scene *s, v3 o, v3 d, float *t)
{
    pto_stats st;
    memset(&st, 0, sizeof st);
    const float of[3] = { o.x, o.y, o.z }, df[3] = { d.x, d.y, d.z };
    return pto_closest(s, of, df, t, &st);
}

static void trace_pixel(const pto_scene *s, const pto_params *p, uint32_t flags, const table_t *T, uint32_t x, uint32_t y, float out[4],
                        double *sq, nr_stats *st)
{
    const uint32_t K = p->streams ? p->streams : 1u;
    const int nee = (flags & NR_NEE) && T->n > 0;
    float accs[MAX_STREAMS][4];
    memset(accs, 0, sizeof accs);
    const uint32_t pixel = y * p->width + x;
    for (uint32_t si = 0; si < p->spp; ++si) {
        float *acc = accs[(p->sample_offset + si) % K];
        float val[3] = { 0.0f, 0.0f, 0.0f }; /* this sample's radiance (variance estimate only) */
        const uint32_t key = pto_path_key(p->seed, pixel, p->sample_offset + si);
        float of[3], df[3];
        pto_camera_ray((const pto_camera *)&s->cam, x, y, key, of, df);
        v3 o = ld3(of), d = ld3(df);
        float Tp[3] = { 1.0f, 1.0f, 1.0f };
        float pb_prev = 0.0f; /* the Lambert pdf of the ray in d (0: a camera ray or one after a specular vertex) */
        uint32_t depth = 0;
        for (;;) {
            float t;
            const uint32_t id = closest(s, o, d, &t);
            st->ext_rays++;
            depth++;
            if (id == PTO_MISS) {
                for (int k = 0; k < 3; ++k) { acc[k] = fma_(Tp[k], s->sky[k], acc[k]); val[k] += Tp[k] * s->sky[k]; }
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
            if (m->emission[0] != 0.0f || m->emission[1] != 0.0f || m->emission[2] != 0.0f) {
                float w = 1.0f; /* w_b: after a Lambert vertex, on a light-set triangle */
                if (nee && pb_prev > 0.0f && id < s->n_tris && T->pa_of[id] > 0.0f && !(flags & NR_NO_MIS)) {
                    const float pl = (T->pa_of[id] * (t * t)) / fabsf(dot3(ng, d)), q = pl / pb_prev;
                    w = nan0(1.0f / fma_(q, q, 1.0f));
                }
                for (int k = 0; k < 3; ++k) {
                    const float e = m->emission[k] * w;
                    acc[k] = fma_(Tp[k], e, acc[k]);
                    val[k] += Tp[k] * e;
                }
            }
            if (depth >= p->max_depth) break;
            const uint32_t b = depth - 1;
            const float u1 = pto_u01(key, 4 + 4 * b), u2 = pto_u01(key, 5 + 4 * b), u3 = pto_u01(key, 6 + 4 * b);
            const float dv[3] = { d.x, d.y, d.z }, nv[3] = { n.x, n.y, n.z };
            float wi[3], W[3], side;
            const int alive = pto_bsdf_sample(m, dv, nv, front, u1, u2, u3, wi, W, &side);
            if (nee && m->kind == PTO_LAMBERT) { /* §7: the light sample of this vertex, with T * albedo of the arriving T */
                const light_t *L = &T->l[pick(T, pto_u01(key, 1024 + 3 * b))];
                const float su = sqrtf(pto_u01(key, 1025 + 3 * b)), b1 = 1.0f - su, b2 = pto_u01(key, 1026 + 3 * b) * su;
                const v3 xl = mk(fma_(b2, L->e2.x, fma_(b1, L->e1.x, L->v0.x)), fma_(b2, L->e2.y, fma_(b1, L->e1.y, L->v0.y)),
                                 fma_(b2, L->e2.z, fma_(b1, L->e1.z, L->v0.z)));
                const v3 so = madd3(p->ray_eps, n, P);
                const v3 dl = sub3(xl, so);
                const float dist2 = dot3(dl, dl), dist = sqrtf(dist2), inv = 1.0f / dist;
                const v3 sd = mk(dl.x * inv, dl.y * inv, dl.z * inv);
                const float cs = dot3(n, sd), cl = fabsf(dot3(L->nl, sd));
                if (cs > 0.0f && cl > 0.0f) {
                    const float pl = (L->pa * dist2) / ((flags & NR_NO_COSL) ? 1.0f : cl), q = (cs * INV_PI) / pl;
                    const float f = (flags & NR_NO_MIS) ? q : nan0(q / fma_(q, q, 1.0f));
                    const float tmax = dist * 0.9999f;
                    float ts;
                    const uint32_t hid = closest(s, so, sd, &ts); /* §4.2 occlusion: blocked iff some intersection has t <= tmax */
                    st->shadow_rays++;
                    if (hid == PTO_MISS || !(ts <= tmax)) {
                        for (int k = 0; k < 3; ++k) {
                            const float Lk = ((Tp[k] * W[k]) * f) * L->le[k];
                            acc[k] = acc[k] + Lk;
                            val[k] += Lk;
                        }
                    }
                }
            }
            if (!alive) break;
            for (int k = 0; k < 3; ++k) Tp[k] = Tp[k] * W[k];
            if (!(fmaxf(Tp[0], fmaxf(Tp[1], Tp[2])) > 0.0f)) break;
            if (depth >= p->rr_start) {
                const float qrr = fminf(fmaxf(Tp[0], fmaxf(Tp[1], Tp[2])), 0.95f);
                if (!(pto_u01(key, 7 + 4 * b) < qrr)) break;
                const float iq = 1.0f / qrr;
                for (int k = 0; k < 3; ++k) Tp[k] = Tp[k] * iq;
            }
            o = madd3(side * p->ray_eps, n, P);
            d = ld3(wi);
            pb_prev = (nee && m->kind == PTO_LAMBERT) ? dot3(n, d) * INV_PI : 0.0f;
        }
        acc[3] += 1.0f;
        st->paths++;
        if (sq) for (int k = 0; k < 3; ++k) sq[k] += (double)val[k] * (double)val[k];
    }
    const float is = 1.0f / (float)p->spp;
    for (int k = 0; k < 4; ++k) {
        float tot = accs[0][k];
        for (uint32_t j = 1; j < K; ++j) tot = tot + accs[j][k];
        out[k] = tot * is;
    }
}

/* rgba: H*W*4 floats; sq (may be NULL): H*W*3 doubles, per pixel and channel the sum over samples of the squared sample radiance */
int nr_render(const pto_scene *s, const pto_params *p, uint32_t flags, int threads, float *rgba, double *sq, nr_stats *st)
{
    if (!s || !p || !rgba || !st || p->spp == 0 || p->streams > MAX_STREAMS) return -1;
    table_t T;
    if (build_table(s, flags, &T) != 0) return -2;
    memset(st, 0, sizeof *st);
    st->n_lights = T.n;
    if (sq) memset(sq, 0, sizeof(double) * 3 * p->width * p->height);
#ifdef _OPENMP
    if (threads > 0) omp_set_num_threads(threads);
#else
    (void)threads;
#endif
    uint64_t ext = 0, shadow = 0, paths = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : ext, shadow, paths)
    for (int y = 0; y < (int)p->height; ++y) {
        nr_stats loc;
        memset(&loc, 0, sizeof loc);
        for (uint32_t x = 0; x < p->width; ++x) {
            const size_t px = (size_t)y * p->width + x;
            trace_pixel(s, p, flags, &T, x, (uint32_t)y, rgba + px * 4, sq ? sq + px * 3 : NULL, &loc);
        }
        ext += loc.ext_rays; shadow += loc.shadow_rays; paths += loc.paths;
    }
    st->ext_rays = ext; st->shadow_rays = shadow; st->paths = paths;
    free(T.l); free(T.cdf); free(T.pa_of);
    return 0;
}
