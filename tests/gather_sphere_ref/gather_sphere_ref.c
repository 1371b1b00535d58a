/*
 * gather_sphere_ref.c — TEST INFRASTRUCTURE ONLY: a scalar restatement of docs/SPEC.md §12.2 with §7.1 (pt_gather_paths with
 * PT_GATHER_PATHS_NEXT_EVENT and, GSR_SPHERES, PT_GATHER_PATHS_SPHERE_LIGHTS), written from the spec and independently of pathtracing_amd/. The pieces §12.2 takes over unchanged come
 * from the oracle (oracle/pt_oracle.h): the RNG, the BSDF sample and the closest hit. Written here: §12's point rule, origin and first
 * direction, §5's loop started at the point, §7's light table and triangle sample, §7.1's joint table and cone sample, §11's map table, lookup, strategy choice and map
 * sample, the MIS weights, the light sample at the point, and §12's lanes, butterfly, division and clamp in plain loops. It links to
 * no other reference of tests/. Nothing in the product may include, link or call this.
 *
 * gsr_gather() reports the rows, the segments and the shadow rays and, for the CPU tests, every sample's radiance.
 * Deliberate errors for the tests' negative controls: GSR_NO_MIS (f = q, w_b = 1), GSR_NO_POINT_SAMPLE (the point takes no light sample,
 * its first ray still carries pb), GSR_NO_COSL (cos_l dropped from the triangle pdf), GSR_NO_PSEL (psel dropped from the pdfs) and
 * GSR_POINT_TW_ALBEDO (the point's term multiplied by the first hit's albedo: "the point is a vertex"); and for the sphere lights
 * GSR_HITS_WEIGHT_1 (hits of sphere lights left at weight 1), GSR_AREA_PDF (the solid-angle pdf of a uniform sample of the whole sphere's
 * area where the cone's stands, both sides) and GSR_SWAP_PMF (the pmf of the first two sphere lights swapped in the pdfs).
 * Without GSR_SPHERES, or on a scene without a sphere light, gsr_gather() is tests/gather_nee_ref's gnr_gather() bit for bit.
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

enum { GSR_NO_MIS = 1, GSR_NO_POINT_SAMPLE = 2, GSR_NO_COSL = 4, GSR_NO_PSEL = 8, GSR_POINT_TW_ALBEDO = 16, GSR_SPHERES = 32, GSR_HITS_WEIGHT_1 = 64,
       GSR_AREA_PDF = 128, GSR_SWAP_PMF = 256 };
typedef struct {
    uint32_t samples, seed, sample_offset, point_offset; /* samples: 1..4096, already resolved (no 0) */
    float max_distance, ray_eps;
    uint32_t max_depth, rr_start;                        /* max_depth: 1..255, already resolved */
} gsr_params;
typedef struct { uint64_t segments, shadow_rays, n_lights, n_sphere_lights; uint32_t lit, pad; } gsr_stats;

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
static int finite_(float x) { return (x - x) == 0.0f; }
#define INV_PI 0.318309873f
#define TWO_PI 6.28318548f
#define MAX_GROUP 64

/* ------------------------------------------------------------------------------------------------ §11: the map and its table */
typedef struct { uint32_t n, lit; float step; float *tex, *mcdf, *ccdf; } env_t; /* tex: r, g, b, p per texel */

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
/* the texel record at encode(d), and s */
static const float *texel_at(const env_t *E, v3 d, float *s_out)
{
    const float s = (fabsf(d.x) + fabsf(d.y)) + fabsf(d.z), is = 1.0f / s, px = d.x * is, py = d.y * is;
    float u = px, v = py;
    if (d.z < 0.0f) { u = (1.0f - fabsf(py)) * sgn(px); v = (1.0f - fabsf(px)) * sgn(py); }
    *s_out = s;
    return E->tex + ((size_t)cell(v, E->n) * E->n + cell(u, E->n)) * 4;
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
static int env_build(const float *rgb, uint32_t n, env_t *E)
{
    const size_t nn = (size_t)n * n;
    memset(E, 0, sizeof *E);
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
    E->lit = total > 0.0;
    double S = 0.0;
    for (uint32_t j = 0; j < n; ++j) {
        S += R[j];
        E->mcdf[j] = (E->lit && j + 1 < n) ? (float)(S / total) : 1.0f;
        double run = 0.0;
        for (uint32_t i = 0; i < n; ++i) {
            const size_t k = (size_t)j * n + i;
            run += w[k];
            E->ccdf[k] = (E->lit && R[j] > 0.0 && i + 1 < n) ? (float)(run / R[j]) : 1.0f;
            memcpy(E->tex + k * 4, rgb + k * 3, 3 * sizeof(float));
            E->tex[k * 4 + 3] = E->lit ? (float)(w[k] / total * ((double)n * (double)n / 4.0)) : 0.0f;
        }
    }
    free(w); free(R);
    return 0;
}

/* ------------------------------------------------------------------------------------------------ §7.1: the cone of a sphere light */
typedef struct { v3 oc; float d2, r2, omc; } cone_t;
static int cone_of(v3 c, float r, v3 o, cone_t *k) /* 0: o is on or inside the sphere */
{
    k->oc = sub3(c, o); k->d2 = dot3(k->oc, k->oc); k->r2 = r * r;
    if (!(k->d2 > k->r2)) return 0;
    const float sin2 = k->r2 / k->d2, cosm = sqrtf(fmaxf(0.0f, 1.0f - sin2));
    k->omc = sin2 / (1.0f + cosm);
    return 1;
}
static v3 cone_dir(const cone_t *k, float u1, float u2, float *thit)
{
    const float z = u1 * k->omc, cos_t = 1.0f - z, s2 = z * (2.0f - z), sin_t = sqrtf(s2);
    float sn, cs;
    pto_sincos2pi(u2, &sn, &cs);
    const float dist = sqrtf(k->d2), inv = 1.0f / dist;
    const v3 w = mk(k->oc.x * inv, k->oc.y * inv, k->oc.z * inv), l = mk(sin_t * cs, sin_t * sn, cos_t);
    *thit = dist * cos_t - sqrtf(fmaxf(0.0f, k->r2 - k->d2 * s2));
    const float sg = copysignf(1.0f, w.z), a = -1.0f / (sg + w.z), b = w.x * w.y * a; /* §5's basis and to_world around w */
    const v3 tx = mk(fma_(sg * w.x, w.x * a, 1.0f), sg * b, -(sg * w.x)), ty = mk(b, fma_(w.y, w.y * a, sg), -w.y);
    return norm3(mk(fma_(l.z, w.x, fma_(l.y, ty.x, l.x * tx.x)), fma_(l.z, w.y, fma_(l.y, ty.y, l.x * tx.y)), fma_(l.z, w.z, fma_(l.y, ty.z, l.x * tx.z))));
}

/* ------------------------------------------------------------------------------------------------ §7 / §7.1: the light table */
typedef struct { int sphere; v3 v0, e1, e2, nl; float pa; v3 c; float r, pmf; uint32_t id; const float *le; } light_t; /* id: which sphere */
typedef struct { uint32_t n, n_tri, n_sph, first2[2]; light_t *l; float *cdf, *pa_of, *pmf_of; } table_t; /* first2: the spheres the first two sphere lights are */

/* spheres: §7.1's joint table (§7's when no sphere is a light); else §7's */
static int table_build(const pto_scene *s, int spheres, table_t *T)
{
    memset(T, 0, sizeof *T);
    const size_t cap = (size_t)s->n_tris + s->n_spheres + 1;
    T->l = calloc(cap, sizeof(light_t)); T->cdf = calloc(cap, sizeof(float)); T->pa_of = calloc(cap, sizeof(float));
    T->pmf_of = calloc(cap, sizeof(float));
    if (!T->pmf_of) return -1;
    double *w = calloc(cap, sizeof(double)), total = 0.0;
    float *area = calloc(cap, sizeof(float));
    uint32_t *id = calloc(cap, sizeof(uint32_t));
    if (!T->l || !T->cdf || !T->pa_of || !w || !area || !id) return -1;
    for (uint32_t i = 0; i < s->n_tris; ++i) {
        const float *e = s->mats[s->tri_mat[i]].emission, *p = s->tri_verts + (size_t)i * 9;
        if (e[0] == 0.0f && e[1] == 0.0f && e[2] == 0.0f) continue;
        light_t Lt;
        memset(&Lt, 0, sizeof Lt);
        Lt.v0 = ld3(p); Lt.e1 = sub3(ld3(p + 3), Lt.v0); Lt.e2 = sub3(ld3(p + 6), Lt.v0);
        const v3 cr = cross3(Lt.e1, Lt.e2);
        const float a = 0.5f * sqrtf(dot3(cr, cr));
        const double wi = (double)a * ((double)e[0] + (double)e[1] + (double)e[2]);
        if (!(a > 0.0f) || !(wi > 0.0)) continue;
        Lt.nl = norm3(cr); Lt.le = e; Lt.pa = 0.0f;
        w[T->n] = wi; area[T->n] = a; id[T->n] = i; T->l[T->n++] = Lt;
    }
    T->n_tri = T->n;
    for (uint32_t j = 0; spheres && j < s->n_spheres; ++j) {
        const float *e = s->mats[s->sph_mat[j]].emission, *sp = s->spheres + (size_t)j * 4;
        if (e[0] == 0.0f && e[1] == 0.0f && e[2] == 0.0f) continue;
        const double wi = (6.283185307179586 * ((double)sp[3] * (double)sp[3])) * (((double)e[0] + (double)e[1]) + (double)e[2]);
        if (!(wi > 0.0)) continue;
        light_t Lt;
        memset(&Lt, 0, sizeof Lt);
        Lt.sphere = 1; Lt.c = ld3(sp); Lt.r = sp[3]; Lt.le = e; Lt.id = j;
        if (T->n - T->n_tri < 2u) T->first2[T->n - T->n_tri] = j;
        w[T->n] = wi; id[T->n] = j; T->l[T->n++] = Lt;
    }
    T->n_sph = T->n - T->n_tri;
    for (uint32_t j = 0; j < T->n; ++j) total += w[j];
    double run = 0.0;
    for (uint32_t j = 0; j < T->n; ++j) {
        run += w[j];
        T->cdf[j] = j + 1 == T->n ? 1.0f : (float)(run / total);
        const float pmf = (float)(w[j] / total);
        if (T->l[j].sphere) { T->l[j].pmf = pmf; T->pmf_of[id[j]] = pmf; }
        else { T->l[j].pa = pmf / area[j]; T->pa_of[id[j]] = T->l[j].pa; }
    }
    free(w); free(area); free(id);
    return 0;
}

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

typedef struct {
    const pto_scene *s; const gsr_params *p; uint32_t flags;
    const table_t *T; const env_t *E;   /* E: NULL without a map */
    int tri_light, env_light;           /* the kinds of light of the call */
    float psel;                         /* as the pdfs use it (1 under GSR_NO_PSEL) */
} call_t;

/* One light sample for a Lambert receiver (normal n, shadow origin so): dimensions dc, dc + 1, dc + 2 and dv of key. Returns 1 if a
 * shadow ray is traced; then f (§7's, Tw not yet in it), le (the light's radiance) and whether it arrived. */
static int light_sample(const call_t *c, uint32_t key, uint32_t dc, uint32_t dv, v3 n, v3 so, float *f, const float **le, int *arrived)
{
    float uc = pto_u01(key, dc);
    int env_branch = c->env_light;
    if (c->env_light && c->tri_light) {
        env_branch = uc < 0.5f;
        uc = env_branch ? uc * 2.0f : fma_(uc, 2.0f, -1.0f);
    }
    v3 wl;
    float tmax;
    uint32_t lamp = PTO_MISS; /* §7.1: the id of the sphere light the shadow ray goes to; what the ray finds of it does not block it */
    if (env_branch) {
        const env_t *E = c->E;
        const uint32_t j = pick(E->mcdf, uc), i = pick(E->ccdf + (size_t)j * E->n, pto_u01(key, dc + 1));
        const float u = fma_((float)i + pto_u01(key, dc + 2), E->step, -1.0f), v = fma_((float)j + pto_u01(key, dv), E->step, -1.0f);
        wl = decode(u, v);
        float s;
        const float *tx = texel_at(E, wl, &s);
        const float cs = dot3(n, wl), pl = c->psel * (tx[3] / ((s * s) * s));
        if (!(cs > 0.0f && pl > 0.0f)) return 0;
        const float q = (cs * INV_PI) / pl;
        *f = (c->flags & GSR_NO_MIS) ? q : nan0(q / fma_(q, q, 1.0f));
        *le = tx; tmax = INFINITY;
    } else if (c->T->l[pick(c->T->cdf, uc)].sphere) { /* §7.1 */
        const uint32_t li = pick(c->T->cdf, uc);
        const light_t *Lt = &c->T->l[li];
        cone_t k;
        if (!cone_of(Lt->c, Lt->r, so, &k)) return 0;
        float thit, pmf = Lt->pmf;
        wl = cone_dir(&k, pto_u01(key, dc + 1), pto_u01(key, dc + 2), &thit);
        float pdfw = 1.0f / (TWO_PI * k.omc);
        if (c->flags & GSR_AREA_PDF) {
            const v3 X = madd3(thit, wl, so), nl = mk((X.x - Lt->c.x) / Lt->r, (X.y - Lt->c.y) / Lt->r, (X.z - Lt->c.z) / Lt->r);
            pdfw = (thit * thit) / (fabsf(dot3(nl, wl)) * (2.0f * TWO_PI * k.r2));
        }
        if ((c->flags & GSR_SWAP_PMF) && c->T->n_sph >= 2 && li < c->T->n_tri + 2u) pmf = c->T->l[li == c->T->n_tri ? li + 1 : li - 1].pmf;
        const float cs = dot3(n, wl), pl = (pmf * c->psel) * pdfw;
        if (!(cs > 0.0f && pl > 0.0f)) return 0;
        const float q = (cs * INV_PI) / pl;
        *f = (c->flags & GSR_NO_MIS) ? q : nan0(q / fma_(q, q, 1.0f));
        *le = Lt->le; tmax = thit * 0.9999f; lamp = c->s->n_tris + Lt->id;
    } else {
        const light_t *Lt = &c->T->l[pick(c->T->cdf, uc)];
        const float su = sqrtf(pto_u01(key, dc + 1)), b1 = 1.0f - su, b2 = pto_u01(key, dc + 2) * su;
        const v3 x = mk(fma_(b2, Lt->e2.x, fma_(b1, Lt->e1.x, Lt->v0.x)), fma_(b2, Lt->e2.y, fma_(b1, Lt->e1.y, Lt->v0.y)),
                        fma_(b2, Lt->e2.z, fma_(b1, Lt->e1.z, Lt->v0.z)));
        const v3 dl = sub3(x, so);
        const float dist2 = dot3(dl, dl), dist = sqrtf(dist2), inv = 1.0f / dist;
        wl = mk(dl.x * inv, dl.y * inv, dl.z * inv);
        const float cs = dot3(n, wl), cl = fabsf(dot3(Lt->nl, wl));
        if (!(cs > 0.0f && cl > 0.0f)) return 0;
        const float pl = ((Lt->pa * c->psel) * dist2) / ((c->flags & GSR_NO_COSL) ? 1.0f : cl), q = (cs * INV_PI) / pl;
        *f = (c->flags & GSR_NO_MIS) ? q : nan0(q / fma_(q, q, 1.0f));
        *le = Lt->le; tmax = dist * 0.9999f;
    }
    float ts;
    const uint32_t hid = closest(c->s, so, wl, &ts); /* §4.2: blocked iff some intersection has t <= tmax */
    *arrived = hid == PTO_MISS || !(ts <= tmax) || hid == lamp;
    return 1;
}

/* One sample. acc[0..2]: the lane's E sums, acc[3..5]: its bent sums, *cnt its count; val[3] the sample's own radiance. */
static void one_sample(const call_t *c, v3 o, v3 nn, uint32_t key, float tmax, float acc[6], uint32_t *cnt, float val[3], uint64_t *segs,
                       uint64_t *shadow)
{
    static const pto_material white = { PTO_LAMBERT, { 1.0f, 1.0f, 1.0f }, { 0.0f, 0.0f, 0.0f }, 0.0f, 1.0f, { 0u, 0u, 0u } };
    const pto_scene *s = c->s;
    const gsr_params *p = c->p;
    const int nee = c->tri_light || c->env_light;
    const float zero[3] = { 0.0f, 0.0f, 0.0f }, nnv[3] = { nn.x, nn.y, nn.z };
    float wi0[3], W0[3], side0;
    pto_bsdf_sample(&white, zero, nnv, 1, pto_u01(key, 0), pto_u01(key, 1), 0.0f, wi0, W0, &side0); /* §5's Lambert sample: its direction */
    v3 d = ld3(wi0);
    float Tp[3] = { 1.0f, 1.0f, 1.0f };
    float pb = nee ? dot3(nn, d) * INV_PI : 0.0f; /* the first ray carries the point's pdf */
    uint32_t depth = 0;
    val[0] = val[1] = val[2] = 0.0f;
    /* the point's light sample: a Lambert receiver with n = nn, Tw = 1, in front of the first segment */
    float pt_term[3] = { 0.0f, 0.0f, 0.0f };
    int pt_pending = 0; /* GSR_POINT_TW_ALBEDO: the term waits for the first hit's albedo */
    if (nee && !(c->flags & GSR_NO_POINT_SAMPLE)) {
        float f;
        const float *le;
        int arrived;
        if (light_sample(c, key, 3072, 3075, nn, o, &f, &le, &arrived)) {
            (*shadow)++;
            if (arrived) {
                for (int k = 0; k < 3; ++k) pt_term[k] = (1.0f * f) * le[k];
                if (c->flags & GSR_POINT_TW_ALBEDO) pt_pending = 1;
                else for (int k = 0; k < 3; ++k) { acc[k] = acc[k] + pt_term[k]; val[k] += pt_term[k]; }
            }
        }
    }
    for (;;) {
        float t;
        const uint32_t id = closest(s, o, d, &t);
        (*segs)++;
        depth++;
        if (depth == 1 && !(id != PTO_MISS && t <= tmax)) { /* §12: V_k = 1, the direction counts for bent */
            acc[3] = acc[3] + d.x; acc[4] = acc[4] + d.y; acc[5] = acc[5] + d.z;
            (*cnt)++;
        }
        if (id == PTO_MISS) {
            if (!c->E) {
                for (int k = 0; k < 3; ++k) { acc[k] = fma_(Tp[k], s->sky[k], acc[k]); val[k] = fma_(Tp[k], s->sky[k], val[k]); }
            } else {
                float sn, w = 1.0f;
                const float *tx = texel_at(c->E, d, &sn);
                if (c->env_light && pb > 0.0f && !(c->flags & GSR_NO_MIS)) {
                    const float pl = c->psel * (tx[3] / ((sn * sn) * sn)), q = pl / pb;
                    w = nan0(1.0f / fma_(q, q, 1.0f));
                }
                for (int k = 0; k < 3; ++k) { const float e = tx[k] * w; acc[k] = fma_(Tp[k], e, acc[k]); val[k] = fma_(Tp[k], e, val[k]); }
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
        if (pt_pending) { /* the deliberate error: the point's term through the first hit's albedo */
            for (int k = 0; k < 3; ++k) { const float Lk = pt_term[k] * m->albedo[k]; acc[k] = acc[k] + Lk; val[k] += Lk; }
            pt_pending = 0;
        }
        if (m->emission[0] != 0.0f || m->emission[1] != 0.0f || m->emission[2] != 0.0f) {
            float w = 1.0f;
            if (c->tri_light && pb > 0.0f && id < s->n_tris && c->T->pa_of[id] > 0.0f && !(c->flags & GSR_NO_MIS)) {
                const float cl = (c->flags & GSR_NO_COSL) ? 1.0f : fabsf(dot3(ng, d));
                const float pl = ((c->T->pa_of[id] * c->psel) * (t * t)) / cl, q = pl / pb;
                w = nan0(1.0f / fma_(q, q, 1.0f));
            }
            if (c->tri_light && pb > 0.0f && id >= s->n_tris && c->T->pmf_of[id - s->n_tris] > 0.0f && !(c->flags & (GSR_NO_MIS | GSR_HITS_WEIGHT_1))) { /* §7.1 */
                const float *sp = s->spheres + (size_t)(id - s->n_tris) * 4;
                cone_t k;
                if (cone_of(ld3(sp), sp[3], o, &k)) {
                    float pdfw = 1.0f / (TWO_PI * k.omc), pmf = c->T->pmf_of[id - s->n_tris];
                    if (c->flags & GSR_AREA_PDF) pdfw = (t * t) / (fabsf(dot3(ng, d)) * (2.0f * TWO_PI * k.r2));
                    if ((c->flags & GSR_SWAP_PMF) && c->T->n_sph >= 2) {
                        if (id - s->n_tris == c->T->first2[0]) pmf = c->T->pmf_of[c->T->first2[1]];
                        else if (id - s->n_tris == c->T->first2[1]) pmf = c->T->pmf_of[c->T->first2[0]];
                    }
                    const float pl = (pmf * c->psel) * pdfw, q = pl / pb;
                    w = nan0(1.0f / fma_(q, q, 1.0f));
                }
            }
            for (int k = 0; k < 3; ++k) { const float e = m->emission[k] * w; acc[k] = fma_(Tp[k], e, acc[k]); val[k] = fma_(Tp[k], e, val[k]); }
        }
        if (depth >= p->max_depth) break;
        const uint32_t b = depth - 1;
        const float u1 = pto_u01(key, 4 + 4 * b), u2 = pto_u01(key, 5 + 4 * b), u3 = pto_u01(key, 6 + 4 * b);
        const float dv[3] = { d.x, d.y, d.z }, nv[3] = { n.x, n.y, n.z };
        float wi[3], W[3], side;
        const int alive = pto_bsdf_sample(m, dv, nv, front, u1, u2, u3, wi, W, &side);
        if (nee && m->kind == PTO_LAMBERT) { /* §7 / §11 at vertex b, whatever the BSDF sample, the black-path test or roulette decide */
            float f;
            const float *le;
            int arrived;
            if (light_sample(c, key, 1024 + 3 * b, 2048 + b, n, madd3(p->ray_eps, n, P), &f, &le, &arrived)) {
                (*shadow)++;
                if (arrived)
                    for (int k = 0; k < 3; ++k) { const float Lk = ((Tp[k] * W[k]) * f) * le[k]; acc[k] = acc[k] + Lk; val[k] += Lk; }
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
        pb = (nee && m->kind == PTO_LAMBERT) ? dot3(n, d) * INV_PI : 0.0f;
    }
}

static void one_point(const call_t *c, const float *rec, uint32_t index, float *out, uint64_t *segs, uint64_t *shadow, float *sample_rad)
{
    const gsr_params *p = c->p;
    const uint32_t K = p->samples;
    const v3 pt = ld3(rec), nv = ld3(rec + 4);
    const float n2 = dot3(nv, nv);
    memset(out, 0, 8 * sizeof(float));
    if (sample_rad) memset(sample_rad, 0, sizeof(float) * 3 * K);
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
            one_sample(c, o, nn, key, tmax, lane[g], &cnt, val, segs, shadow);
            if (sample_rad) memcpy(sample_rad + 3 * (size_t)k, val, sizeof val);
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

/* points, out: n records of 8 floats. env (may be NULL): env_n * env_n * 3 floats, row-major. sample_rad (may be NULL): n * K * 3 floats. */
int gsr_gather(const pto_scene *s, const float *env, uint32_t env_n, const gsr_params *p, uint32_t flags, int threads, const float *points,
               uint64_t n, float *out, gsr_stats *st, float *sample_rad)
{
    if (!s || !p || !points || !out || !st || p->samples == 0 || p->samples > 4096 || p->max_depth == 0 || p->max_depth > 255 || (env && !env_n)) return -1;
    table_t T;
    env_t E;
    if (table_build(s, (flags & GSR_SPHERES) != 0, &T) != 0) return -2;
    memset(&E, 0, sizeof E);
    if (env && env_build(env, env_n, &E) != 0) return -2;
    call_t c;
    c.s = s; c.p = p; c.flags = flags; c.T = &T; c.E = env ? &E : NULL;
    c.tri_light = T.n > 0; c.env_light = env && E.lit;
    c.psel = (c.tri_light && c.env_light && !(flags & GSR_NO_PSEL)) ? 0.5f : 1.0f;
#ifdef _OPENMP
    if (threads > 0) omp_set_num_threads(threads);
#else
    (void)threads;
#endif
    uint64_t segs = 0, shadow = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : segs, shadow)
    for (long long i = 0; i < (long long)n; ++i) {
        uint64_t a = 0, b = 0;
        one_point(&c, points + 8 * (size_t)i, (uint32_t)i, out + 8 * (size_t)i, &a, &b, sample_rad ? sample_rad + 3 * (size_t)i * p->samples : NULL);
        segs += a; shadow += b;
    }
    memset(st, 0, sizeof *st);
    st->segments = segs; st->shadow_rays = shadow; st->n_lights = T.n_tri; st->n_sphere_lights = T.n_sph; st->lit = E.lit;
    free(T.l); free(T.cdf); free(T.pa_of); free(T.pmf_of); free(E.tex); free(E.mcdf); free(E.ccdf);
    return 0;
}
