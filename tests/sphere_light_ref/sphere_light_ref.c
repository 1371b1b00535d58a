/*
 * sphere_light_ref.c — TEST INFRASTRUCTURE ONLY: a scalar restatement of docs/SPEC.md §7.1 (sphere lights) together with the §5 path loop,
 * the §7 light sample and the §11 environment it sits in, written from the spec and independently of pathtracing_amd/. The pieces those
 * sections take over unchanged come from the oracle (oracle/pt_oracle.h): the closest hit, the BSDF sample, the pinhole camera ray and the
 * RNG. A lens ray (§3.1) comes from the caller as a function — tests/lens_ref's lr_camera_ray — so a frame through a lens composes with
 * that checker's rule. The joint table, the cone, both light samples, the MIS weights and the accumulation are written here.
 * Nothing in the product may include, link or call this.
 *
 * sl_render() with flags = 0 is §5 (pto_render bit for bit), with SL_NEE §7 / §11 (nee_ref / env_ref bit for bit), with SL_NEE |
 * SL_SPHERES §7.1. The rest are deliberate errors for the tests' negative controls: SL_HITS_WEIGHT_1 leaves hits of sphere lights at
 * weight 1, SL_AREA_PDF puts the solid-angle pdf of a uniform sample of the whole sphere's area where the cone's stands (both sides),
 * SL_SWAP_PMF swaps the pmf of the first two sphere lights in the pdfs, SL_NO_PSEL drops psel from the pdfs, SL_NAIVE_OMC computes
 * 1 - cos(theta_max) as 1.0f - cosm, SL_LAMP_BLOCKS lets what a shadow ray finds of its own lamp block it.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif
#include "../../oracle/pt_oracle.h"

enum { SL_NEE = 1, SL_SPHERES = 2, SL_HITS_WEIGHT_1 = 4, SL_AREA_PDF = 8, SL_SWAP_PMF = 16, SL_NO_PSEL = 32, SL_NAIVE_OMC = 64, SL_LAMP_BLOCKS = 128 };
typedef struct { uint64_t ext_rays, shadow_rays, paths, n_lights, n_sphere_lights; uint32_t lit, pad; } sl_stats;
typedef struct { float radius, focus_distance; } sl_lens;
/* tests/lens_ref: lr_camera_ray(camera, lens, w, h, x, y, key, o, d); w = 0: the frame was accepted already */
typedef int (*sl_lens_ray_fn)(const pto_camera *, const sl_lens *, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, float *, float *);

typedef struct { float x, y, z; } v3;
static inline v3 mk(float x, float y, float z) { v3 r = { x, y, z }; return r; }
static inline float fma_(float a, float b, float c) { return fmaf(a, b, c); }
static inline float dot3(v3 a, v3 b) { return fma_(a.z, b.z, fma_(a.y, b.y, a.x * b.x)); }
static inline v3 cross3(v3 a, v3 b) { return mk(fma_(a.y, b.z, -(a.z * b.y)), fma_(a.z, b.x, -(a.x * b.z)), fma_(a.x, b.y, -(a.y * b.x))); }
static inline v3 sub3(v3 a, v3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
static inline v3 madd3(float t, v3 d, v3 o) { return mk(fma_(t, d.x, o.x), fma_(t, d.y, o.y), fma_(t, d.z, o.z)); }
static inline v3 ld3(const float *p) { return mk(p[0], p[1], p[2]); }
static inline v3 norm3(v3 v) { float s = 1.0f / sqrtf(dot3(v, v)); return mk(v.x * s, v.y * s, v.z * s); }
static inline float nan0(float w) { return w >= 0.0f ? w : 0.0f; }
static inline float sgn(float x) { return copysignf(1.0f, x); }
#define INV_PI 0.318309873f
#define TWO_PI 6.28318548f
#define MAX_STREAMS 64

/* ------------------------------------------------------------------------------------------------ §7.1 the cone */
typedef struct { v3 oc; float d2, r2, omc, cosm; } cone_t;

/* 0: o is on or inside the sphere */
static int cone_of(v3 c, float r, v3 o, uint32_t flags, cone_t *k)
{
    k->oc = sub3(c, o); k->d2 = dot3(k->oc, k->oc); k->r2 = r * r;
    if (!(k->d2 > k->r2)) return 0;
    const float sin2 = k->r2 / k->d2;
    k->cosm = sqrtf(fmaxf(0.0f, 1.0f - sin2));
    k->omc = (flags & SL_NAIVE_OMC) ? 1.0f - k->cosm : sin2 / (1.0f + k->cosm);
    return 1;
}
static float cone_pdf(const cone_t *k) { return 1.0f / (TWO_PI * k->omc); }

/* §5's basis and to_world around w */
static v3 around(v3 w, v3 l)
{
    const float sg = copysignf(1.0f, w.z), a = -1.0f / (sg + w.z), b = w.x * w.y * a;
    const v3 tx = mk(fma_(sg * w.x, w.x * a, 1.0f), sg * b, -(sg * w.x)), ty = mk(b, fma_(w.y, w.y * a, sg), -w.y);
    return norm3(mk(fma_(l.z, w.x, fma_(l.y, ty.x, l.x * tx.x)), fma_(l.z, w.y, fma_(l.y, ty.y, l.x * tx.y)), fma_(l.z, w.z, fma_(l.y, ty.z, l.x * tx.z))));
}

static v3 cone_dir(const cone_t *k, float u1, float u2, float *thit)
{
    const float z = u1 * k->omc, cos_t = 1.0f - z, s2 = z * (2.0f - z), sin_t = sqrtf(s2);
    float sn, cs;
    pto_sincos2pi(u2, &sn, &cs);
    const float dist = sqrtf(k->d2), inv = 1.0f / dist;
    const v3 w = mk(k->oc.x * inv, k->oc.y * inv, k->oc.z * inv);
    *thit = dist * cos_t - sqrtf(fmaxf(0.0f, k->r2 - k->d2 * s2));
    return around(w, mk(sin_t * cs, sin_t * sn, cos_t));
}

/* for the numerics test: out = omc, pdf_w, thit, wl.xyz, cosm, dot(wl, oc/|oc|); returns 0 when o is on or inside the sphere */
int sl_cone(const float c[3], float r, const float o[3], float u1, float u2, uint32_t flags, float out[8])
{
    cone_t k;
    if (!cone_of(ld3(c), r, ld3(o), flags, &k)) return 0;
    float thit;
    const v3 wl = cone_dir(&k, u1, u2, &thit);
    const float inv = 1.0f / sqrtf(k.d2);
    out[0] = k.omc; out[1] = cone_pdf(&k); out[2] = thit; out[3] = wl.x; out[4] = wl.y; out[5] = wl.z; out[6] = k.cosm;
    out[7] = dot3(wl, mk(k.oc.x * inv, k.oc.y * inv, k.oc.z * inv));
    return 1;
}

/* ------------------------------------------------------------------------------------------------ §11 map (as tests/env_ref/) */
static v3 decode(float u, float v)
{
    const float z = (1.0f - fabsf(u)) - fabsf(v);
    float x = u, y = v;
    if (z < 0.0f) { x = (1.0f - fabsf(v)) * sgn(u); y = (1.0f - fabsf(u)) * sgn(v); }
    return norm3(mk(x, y, z));
}
static uint32_t cell(float u, uint32_t n)
{
    int i = (int)floorf(fma_(u, 0.5f, 0.5f) * (float)n);
    if (i < 0) i = 0;
    if (i > (int)n - 1) i = (int)n - 1;
    return (uint32_t)i;
}
static double centre_norm1(uint32_t i, uint32_t j, uint32_t n)
{
    const double u = (double)(2u * i + 1u) / (double)n - 1.0, v = (double)(2u * j + 1u) / (double)n - 1.0;
    const double z = (1.0 - fabs(u)) - fabs(v);
    double x = u, y = v;
    if (z < 0.0) { x = (1.0 - fabs(v)) * copysign(1.0, u); y = (1.0 - fabs(u)) * copysign(1.0, v); }
    const double len = sqrt((x * x + y * y) + z * z);
    return (fabs(x / len) + fabs(y / len)) + fabs(z / len);
}
typedef struct { uint32_t n, lit; float step; float *tex, *mcdf, *ccdf; } env_t;

static int env_table(const float *rgb, uint32_t n, env_t *E)
{
    const size_t nn = (size_t)n * n;
    E->n = n; E->step = 2.0f / (float)n;
    E->tex = malloc(sizeof(float) * 4 * nn); E->mcdf = malloc(sizeof(float) * n); E->ccdf = malloc(sizeof(float) * nn);
    double *w = malloc(sizeof(double) * nn), *R = malloc(sizeof(double) * n), total = 0.0;
    if (!E->tex || !E->mcdf || !E->ccdf || !w || !R) return -1;
    for (uint32_t j = 0; j < n; ++j) {
        double row = 0.0;
        for (uint32_t i = 0; i < n; ++i) {
            const float *c = rgb + ((size_t)j * n + i) * 3;
            const double sc = centre_norm1(i, j, n);
            w[(size_t)j * n + i] = ((double)c[0] + (double)c[1] + (double)c[2]) * ((sc * sc) * sc);
            row += w[(size_t)j * n + i];
        }
        R[j] = row; total += row;
    }
    const int lit = total > 0.0;
    double S = 0.0;
    const double scale = (double)n * (double)n / 4.0;
    for (uint32_t j = 0; j < n; ++j) {
        S += R[j];
        E->mcdf[j] = (lit && j + 1 < n) ? (float)(S / total) : 1.0f;
        double run = 0.0;
        for (uint32_t i = 0; i < n; ++i) {
            const size_t k = (size_t)j * n + i;
            run += w[k];
            E->ccdf[k] = (lit && R[j] > 0.0 && i + 1 < n) ? (float)(run / R[j]) : 1.0f;
            E->tex[k * 4 + 0] = rgb[k * 3 + 0]; E->tex[k * 4 + 1] = rgb[k * 3 + 1]; E->tex[k * 4 + 2] = rgb[k * 3 + 2];
            E->tex[k * 4 + 3] = lit ? (float)(w[k] / total * scale) : 0.0f;
        }
    }
    free(w); free(R);
    E->lit = (uint32_t)lit;
    return 0;
}
/* the texel record at encode(d) and the solid-angle pdf there */
static const float *lookup(const env_t *E, v3 d, float *pdf)
{
    const float s = (fabsf(d.x) + fabsf(d.y)) + fabsf(d.z), is = 1.0f / s, px = d.x * is, py = d.y * is;
    float u = px, v = py;
    if (d.z < 0.0f) { u = (1.0f - fabsf(py)) * sgn(px); v = (1.0f - fabsf(px)) * sgn(py); }
    const float *tx = E->tex + ((size_t)cell(v, E->n) * E->n + cell(u, E->n)) * 4;
    *pdf = tx[3] / ((s * s) * s);
    return tx;
}

/* ------------------------------------------------------------------------------------------------ §7 / §7.1 light table */
typedef struct { int sphere; v3 v0, e1, e2, nl; float area, pmf, pa; v3 c; float r; uint32_t id; const float *le; } light_t; /* id: which sphere */
typedef struct { uint32_t n, n_tri, n_sph; light_t *l; float *cdf; float *pa_of, *pmf_of; } table_t;

/* spheres: the joint table of §7.1 (which is §7's when no sphere is a light); else §7's */
static int build_table(const pto_scene *s, int spheres, table_t *T)
{
    memset(T, 0, sizeof *T);
    const size_t cap = (size_t)s->n_tris + s->n_spheres + 1;
    T->l = calloc(cap, sizeof(light_t)); T->cdf = calloc(cap, sizeof(float));
    T->pa_of = calloc(s->n_tris + 1, sizeof(float)); T->pmf_of = calloc(s->n_spheres + 1, sizeof(float));
    double *w = calloc(cap, sizeof(double)), total = 0.0;
    uint32_t *id = calloc(cap, sizeof(uint32_t));
    if (!T->l || !T->cdf || !T->pa_of || !T->pmf_of || !w || !id) return -1;
    for (uint32_t i = 0; i < s->n_tris; ++i) {
        const float *e = s->mats[s->tri_mat[i]].emission;
        if (e[0] == 0.0f && e[1] == 0.0f && e[2] == 0.0f) continue;
        const float *p = s->tri_verts + (size_t)i * 9;
        light_t L;
        memset(&L, 0, sizeof L);
        L.v0 = ld3(p); L.e1 = sub3(ld3(p + 3), L.v0); L.e2 = sub3(ld3(p + 6), L.v0);
        const v3 cr = cross3(L.e1, L.e2);
        L.area = 0.5f * sqrtf(dot3(cr, cr));
        const double wi = (double)L.area * ((double)e[0] + (double)e[1] + (double)e[2]);
        if (!(L.area > 0.0f) || !(wi > 0.0)) continue;
        L.nl = norm3(cr); L.le = e;
        w[T->n] = wi; id[T->n] = i; T->l[T->n++] = L;
    }
    T->n_tri = T->n;
    for (uint32_t j = 0; spheres && j < s->n_spheres; ++j) {
        const float *e = s->mats[s->sph_mat[j]].emission, *sp = s->spheres + (size_t)j * 4;
        if (e[0] == 0.0f && e[1] == 0.0f && e[2] == 0.0f) continue;
        const double wi = (6.283185307179586 * ((double)sp[3] * (double)sp[3])) * (((double)e[0] + (double)e[1]) + (double)e[2]);
        if (!(wi > 0.0)) continue;
        light_t L;
        memset(&L, 0, sizeof L);
        L.sphere = 1; L.c = ld3(sp); L.r = sp[3]; L.le = e; L.id = j;
        w[T->n] = wi; id[T->n] = j; T->l[T->n++] = L;
    }
    T->n_sph = T->n - T->n_tri;
    for (uint32_t j = 0; j < T->n; ++j) total += w[j];
    double run = 0.0;
    for (uint32_t j = 0; j < T->n; ++j) {
        run += w[j];
        T->cdf[j] = j + 1 == T->n ? 1.0f : (float)(run / total);
        T->l[j].pmf = (float)(w[j] / total);
        if (T->l[j].sphere) T->pmf_of[id[j]] = T->l[j].pmf;
        else { T->l[j].pa = T->l[j].pmf / T->l[j].area; T->pa_of[id[j]] = T->l[j].pa; }
    }
    free(w); free(id);
    return 0;
}
static void free_table(table_t *T) { free(T->l); free(T->cdf); free(T->pa_of); free(T->pmf_of); }

static uint32_t pick(const float *cdf, float u)
{
    uint32_t i = 0;
    while (!(u < cdf[i])) ++i; /* the smallest i with u < cdf[i]; the last entry is 1 > u */
    return i;
}

static uint32_t closest(const pto_scene *s, v3 o, v3 d, float *t)
{
    pto_stats st;
    memset(&st, 0, sizeof st);
    const float of[3] = { o.x, o.y, o.z }, df[3] = { d.x, d.y, d.z };
    return pto_closest(s, of, df, t, &st);
}

/* SL_SWAP_PMF: the pmf the pdfs use for sphere `j` of the scene — the other one's, for the first two sphere lights */
static float pmf_used(const pto_scene *s, const table_t *T, uint32_t j, uint32_t flags)
{
    if ((flags & SL_SWAP_PMF) && T->n_sph >= 2) {
        uint32_t a = 0, b = 0, seen = 0;
        for (uint32_t k = 0; k < s->n_spheres && seen < 2; ++k)
            if (T->pmf_of[k] > 0.0f) { if (seen++ == 0) a = k; else b = k; }
        if (j == a) return T->pmf_of[b];
        if (j == b) return T->pmf_of[a];
    }
    return T->pmf_of[j];
}

typedef struct { const sl_lens *lens; sl_lens_ray_fn ray; } lens_t;

static void trace_pixel(const pto_scene *s, const pto_params *p, uint32_t flags, const table_t *T, const env_t *E, const lens_t *ln,
                        uint32_t x, uint32_t y, float out[4], double *sq, sl_stats *st)
{
    const uint32_t K = p->streams ? p->streams : 1u;
    const int env_light = (flags & SL_NEE) && E && E->lit, tab_light = (flags & SL_NEE) && T->n > 0;
    const int nee = env_light || tab_light;
    const float psel_true = (env_light && tab_light) ? 0.5f : 1.0f, psel = (flags & SL_NO_PSEL) ? 1.0f : psel_true;
    float accs[MAX_STREAMS][4];
    memset(accs, 0, sizeof accs);
    const uint32_t pixel = y * p->width + x;
    for (uint32_t si = 0; si < p->spp; ++si) {
        float *acc = accs[(p->sample_offset + si) % K];
        float val[3] = { 0.0f, 0.0f, 0.0f };
        const uint32_t key = pto_path_key(p->seed, pixel, p->sample_offset + si);
        float of[3], df[3];
        if (ln) ln->ray((const pto_camera *)&s->cam, ln->lens, 0u, 0u, x, y, key, of, df);
        else pto_camera_ray((const pto_camera *)&s->cam, x, y, key, of, df);
        v3 o = ld3(of), d = ld3(df);
        float Tp[3] = { 1.0f, 1.0f, 1.0f };
        float pb_prev = 0.0f;
        uint32_t depth = 0;
        for (;;) {
            float t;
            const uint32_t id = closest(s, o, d, &t);
            st->ext_rays++;
            depth++;
            if (id == PTO_MISS) {
                if (!E) {
                    for (int k = 0; k < 3; ++k) { acc[k] = fma_(Tp[k], s->sky[k], acc[k]); val[k] += Tp[k] * s->sky[k]; }
                } else {
                    float pdf, w = 1.0f;
                    const float *tx = lookup(E, d, &pdf);
                    if (env_light && pb_prev > 0.0f) {
                        const float pl = psel * pdf, q = pl / pb_prev;
                        w = nan0(1.0f / fma_(q, q, 1.0f));
                    }
                    for (int k = 0; k < 3; ++k) { const float e = tx[k] * w; acc[k] = fma_(Tp[k], e, acc[k]); val[k] += Tp[k] * e; }
                }
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
                float w = 1.0f;
                if (tab_light && pb_prev > 0.0f && id < s->n_tris && T->pa_of[id] > 0.0f) { /* §7 w_b, with the table's (joint) pa */
                    const float pl = ((T->pa_of[id] * psel) * (t * t)) / fabsf(dot3(ng, d)), q = pl / pb_prev;
                    w = nan0(1.0f / fma_(q, q, 1.0f));
                }
                if (tab_light && pb_prev > 0.0f && id >= s->n_tris && T->pmf_of[id - s->n_tris] > 0.0f && !(flags & SL_HITS_WEIGHT_1)) { /* §7.1 */
                    const float *sp = s->spheres + (size_t)(id - s->n_tris) * 4;
                    cone_t k;
                    if (cone_of(ld3(sp), sp[3], o, flags, &k)) {
                        float pdfw = cone_pdf(&k);
                        if (flags & SL_AREA_PDF) pdfw = (t * t) / (fabsf(dot3(ng, d)) * (2.0f * TWO_PI * k.r2));
                        const float pl = (pmf_used(s, T, id - s->n_tris, flags) * psel) * pdfw, q = pl / pb_prev;
                        w = nan0(1.0f / fma_(q, q, 1.0f));
                    }
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
            if (nee && m->kind == PTO_LAMBERT) {
                float uc = pto_u01(key, 1024 + 3 * b);
                int env_branch = env_light;
                if (env_light && tab_light) {
                    env_branch = uc < 0.5f;
                    uc = env_branch ? uc * 2.0f : fma_(uc, 2.0f, -1.0f);
                }
                const v3 so = madd3(p->ray_eps, n, P);
                int traced = 0;
                uint32_t lamp = PTO_MISS; /* §7.1: the id of the sphere light the shadow ray goes to; what the ray finds of it does not block it */
                v3 sd = mk(0, 0, 0);
                float f = 0.0f, tmax = 0.0f;
                const float *le = NULL;
                if (env_branch) {
                    const uint32_t j = pick(E->mcdf, uc), i = pick(E->ccdf + (size_t)j * E->n, pto_u01(key, 1025 + 3 * b));
                    const float u = fma_((float)i + pto_u01(key, 1026 + 3 * b), E->step, -1.0f);
                    const float v = fma_((float)j + pto_u01(key, 2048 + b), E->step, -1.0f);
                    sd = decode(u, v);
                    float pdf;
                    const float *tx = lookup(E, sd, &pdf);
                    const float cs = dot3(n, sd), pl = psel * pdf;
                    if (cs > 0.0f && pl > 0.0f) {
                        const float q = (cs * INV_PI) / pl;
                        f = nan0(q / fma_(q, q, 1.0f));
                        traced = 1; tmax = INFINITY; le = tx;
                    }
                } else {
                    const uint32_t li = pick(T->cdf, uc);
                    const light_t *L = &T->l[li];
                    if (L->sphere) { /* §7.1 */
                        cone_t k;
                        if (cone_of(L->c, L->r, so, flags, &k)) {
                            float thit;
                            sd = cone_dir(&k, pto_u01(key, 1025 + 3 * b), pto_u01(key, 1026 + 3 * b), &thit);
                            float pdfw = cone_pdf(&k), pmf = L->pmf;
                            if (flags & SL_AREA_PDF) {
                                const v3 X = madd3(thit, sd, so);
                                const v3 nl = mk((X.x - L->c.x) / L->r, (X.y - L->c.y) / L->r, (X.z - L->c.z) / L->r);
                                pdfw = (thit * thit) / (fabsf(dot3(nl, sd)) * (2.0f * TWO_PI * k.r2));
                            }
                            if ((flags & SL_SWAP_PMF) && T->n_sph >= 2 && li < T->n_tri + 2u) pmf = T->l[li == T->n_tri ? li + 1 : li - 1].pmf;
                            const float cs = dot3(n, sd), pl = (pmf * psel) * pdfw;
                            if (cs > 0.0f && pl > 0.0f) {
                                const float q = (cs * INV_PI) / pl;
                                f = nan0(q / fma_(q, q, 1.0f));
                                traced = 1; tmax = thit * 0.9999f; le = L->le; lamp = s->n_tris + L->id;
                            }
                        }
                    } else {
                        const float su = sqrtf(pto_u01(key, 1025 + 3 * b)), b1 = 1.0f - su, b2 = pto_u01(key, 1026 + 3 * b) * su;
                        const v3 xl = mk(fma_(b2, L->e2.x, fma_(b1, L->e1.x, L->v0.x)), fma_(b2, L->e2.y, fma_(b1, L->e1.y, L->v0.y)),
                                         fma_(b2, L->e2.z, fma_(b1, L->e1.z, L->v0.z)));
                        const v3 dl = sub3(xl, so);
                        const float dist2 = dot3(dl, dl), dist = sqrtf(dist2), inv = 1.0f / dist;
                        sd = mk(dl.x * inv, dl.y * inv, dl.z * inv);
                        const float cs = dot3(n, sd), cl = fabsf(dot3(L->nl, sd));
                        if (cs > 0.0f && cl > 0.0f) {
                            const float pl = ((L->pa * psel) * dist2) / cl, q = (cs * INV_PI) / pl;
                            f = nan0(q / fma_(q, q, 1.0f));
                            traced = 1; tmax = dist * 0.9999f; le = L->le;
                        }
                    }
                }
                if (traced) {
                    float ts;
                    const uint32_t hid = closest(s, so, sd, &ts); /* §4.2: blocked iff some intersection has t <= tmax */
                    st->shadow_rays++;
                    if (hid == PTO_MISS || !(ts <= tmax) || (hid == lamp && !(flags & SL_LAMP_BLOCKS))) {
                        for (int k = 0; k < 3; ++k) {
                            const float Lk = ((Tp[k] * W[k]) * f) * le[k];
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

/* env_rgb (may be NULL: no environment, misses add the scene's sky): env_n * env_n * 3 floats. lens / lens_ray (may both be NULL: the
 * pinhole camera): the lens and tests/lens_ref's lr_camera_ray. rgba: H*W*4 floats; sq (may be NULL): H*W*3 doubles, per pixel and
 * channel the sum over samples of the squared sample radiance */
int sl_render(const pto_scene *s, const pto_params *p, const float *env_rgb, uint32_t env_n, const sl_lens *lens, sl_lens_ray_fn lens_ray,
              uint32_t flags, int threads, float *rgba, double *sq, sl_stats *st)
{
    if (!s || !p || !rgba || !st || p->spp == 0 || p->streams > MAX_STREAMS || (env_rgb && env_n == 0) || (!lens != !lens_ray)) return -1;
    if ((flags & SL_SPHERES) && !(flags & SL_NEE)) return -3; /* refused, as PT_FLAG_NEXT_EVENT_SPHERES alone is */
    table_t T;
    if (build_table(s, (flags & SL_SPHERES) != 0, &T) != 0) return -2;
    env_t E;
    memset(&E, 0, sizeof E);
    if (env_rgb && env_table(env_rgb, env_n, &E) != 0) return -2;
    lens_t ln = { lens, lens_ray };
    if (lens) { /* a refused lens: before anything is traced */
        float o[3], d[3];
        if (lens_ray((const pto_camera *)&s->cam, lens, p->width, p->height, 0u, 0u, 0u, o, d) != 0) { free_table(&T); return -4; }
    }
    memset(st, 0, sizeof *st);
    st->n_lights = T.n_tri; st->n_sphere_lights = T.n_sph; st->lit = E.lit;
    if (sq) memset(sq, 0, sizeof(double) * 3 * p->width * p->height);
#ifdef _OPENMP
    if (threads > 0) omp_set_num_threads(threads);
#else
    (void)threads;
#endif
    uint64_t ext = 0, shadow = 0, paths = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : ext, shadow, paths)
    for (int y = 0; y < (int)p->height; ++y) {
        sl_stats loc;
        memset(&loc, 0, sizeof loc);
        for (uint32_t x = 0; x < p->width; ++x) {
            const size_t px = (size_t)y * p->width + x;
            trace_pixel(s, p, flags, &T, env_rgb ? &E : NULL, lens ? &ln : NULL, x, (uint32_t)y, rgba + px * 4, sq ? sq + px * 3 : NULL, &loc);
        }
        ext += loc.ext_rays; shadow += loc.shadow_rays; paths += loc.paths;
    }
    st->ext_rays = ext; st->shadow_rays = shadow; st->paths = paths;
    free_table(&T); free(E.tex); free(E.mcdf); free(E.ccdf);
    return 0;
}
