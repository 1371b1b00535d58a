/*
 * tex_ref.c — TEST INFRASTRUCTURE ONLY: a scalar restatement of docs/SPEC.md §13 (albedo textures) together with the §5 path loop, the §7
 * light sample and the §11 environment map it sits in, written from the spec and independently of pathtracing_amd/. The pieces those
 * sections take over unchanged come from the oracle (oracle/pt_oracle.h): the closest hit, the BSDF sample, the camera ray and the RNG.
 * The barycentrics of the winning triangle, the coordinate, the wrap, both lookups and where the effective albedo enters the loop are
 * written here; the loop around them is the one tests/env_ref/ holds to the oracle. Nothing in the product may include, link or call this.
 *
 * tr_render() without textures, without an environment and with flags = 0 is §5 (pto_render bit for bit), with TR_NEE §7.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif
#include "../../oracle/pt_oracle.h"

enum { TR_NEE = 1 };
enum { TR_TEXTURE_NEAREST = 1 };
#define TR_NO_TEXTURE 0xFFFFFFFFu
typedef struct { uint64_t ext_rays, shadow_rays, paths, n_lights; uint32_t lit, pad; } tr_stats;
typedef struct { uint32_t width, height, flags, pad; const float *rgb; } tr_texture; /* rgb: height rows of width texels, 3 floats each */
typedef struct {
    const float *uv6;            /* 6 floats per triangle, or NULL: no UVs */
    const tr_texture *tex;       /* n_tex textures; width 0 = not set */
    uint32_t n_tex, pad;
    const uint32_t *of_material; /* per material a texture index or TR_NO_TEXTURE, or NULL: no binding */
} tr_textures;

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
#define MAX_STREAMS 64

/* ------------------------------------------------------------------------------------------------ §13 */
/* one axis of the bilinear lookup: the two texel indices and the weight from the wrapped coordinate f */
static void axis(float f, uint32_t n, uint32_t *i0, uint32_t *i1, float *w)
{
    const float xf = fma_(f, (float)n, -0.5f), x0f = floorf(xf);
    *w = xf - x0f;
    int a = (int)x0f, b = a + 1;
    if (a < 0) a += (int)n;
    if (b >= (int)n) b -= (int)n;
    *i0 = (uint32_t)a; *i1 = (uint32_t)b;
}

void tr_lookup(const tr_texture *T, float s, float t, float out[3])
{
    const float fs = s - floorf(s), ft = t - floorf(t);
    const uint32_t W = T->width, H = T->height;
    if (T->flags & TR_TEXTURE_NEAREST) {
        int x = (int)floorf(fs * (float)W), y = (int)floorf(ft * (float)H);
        if (x > (int)W - 1) x = (int)W - 1;
        if (y > (int)H - 1) y = (int)H - 1;
        const float *c = T->rgb + ((size_t)y * W + (size_t)x) * 3;
        out[0] = c[0]; out[1] = c[1]; out[2] = c[2];
        return;
    }
    uint32_t x0, x1, y0, y1;
    float fx, fy;
    axis(fs, W, &x0, &x1, &fx); axis(ft, H, &y0, &y1, &fy);
    const float *a = T->rgb + ((size_t)y0 * W + x0) * 3, *b = T->rgb + ((size_t)y0 * W + x1) * 3;
    const float *p = T->rgb + ((size_t)y1 * W + x0) * 3, *q = T->rgb + ((size_t)y1 * W + x1) * 3;
    for (int k = 0; k < 3; ++k) {
        const float top = fma_(fx, b[k] - a[k], a[k]), bot = fma_(fx, q[k] - p[k], p[k]);
        out[k] = fma_(fy, bot - top, top);
    }
}

/* §4's (u, v) of the ray (o, d) on the triangle v9 = v0, v1, v2 */
void tr_barycentrics(const float v9[9], const float of[3], const float df[3], float uv[2])
{
    const v3 v0 = ld3(v9), e1 = sub3(ld3(v9 + 3), v0), e2 = sub3(ld3(v9 + 6), v0), o = ld3(of), d = ld3(df);
    const v3 p = cross3(d, e2);
    const float inv_det = 1.0f / dot3(e1, p);
    const v3 tv = sub3(o, v0);
    uv[0] = dot3(tv, p) * inv_det;
    uv[1] = dot3(d, cross3(tv, e1)) * inv_det;
}

/* the coordinate of barycentrics (u, v) on a triangle with uv6 = s0, t0, s1, t1, s2, t2 */
void tr_coordinate(const float uv6[6], float u, float v, float st[2])
{
    const float w0 = (1.0f - u) - v;
    st[0] = fma_(v, uv6[4], fma_(u, uv6[2], w0 * uv6[0]));
    st[1] = fma_(v, uv6[5], fma_(u, uv6[3], w0 * uv6[1]));
}

/* tr_coordinate and tr_lookup over n points, for tests that ask a few hundred thousand times: plain loops, no arithmetic of their own.
 * uv6: 6 floats per point; st: 2 per point; out: 3 per point. */
void tr_coordinate_many(const float *uv6, const float *u, const float *v, size_t n, float *st)
{
    for (size_t i = 0; i < n; ++i) tr_coordinate(uv6 + i * 6, u[i], v[i], st + i * 2);
}

void tr_lookup_many(const tr_texture *T, const float *st, size_t n, float *out)
{
    for (size_t i = 0; i < n; ++i) tr_lookup(T, st[i * 2], st[i * 2 + 1], out + i * 3);
}

/* the texture a hit of triangle `id` looks up, or NULL */
static const tr_texture *texture_of(const pto_scene *s, const tr_textures *X, uint32_t id)
{
    if (!X || !X->uv6 || !X->of_material) return NULL;
    const uint32_t t = X->of_material[s->tri_mat[id]];
    if (t == TR_NO_TEXTURE || t >= X->n_tex || X->tex[t].width == 0) return NULL;
    return &X->tex[t];
}

/* albedo * texel of a hit of triangle `id` by the ray (o, d), if the triangle's material is bound; else the albedo. Returns 1 if textured. */
static int effective_albedo(const pto_scene *s, const tr_textures *X, uint32_t id, v3 o, v3 d, const float albedo[3], float out[3])
{
    out[0] = albedo[0]; out[1] = albedo[1]; out[2] = albedo[2];
    const tr_texture *T = texture_of(s, X, id);
    if (!T) return 0;
    const float of[3] = { o.x, o.y, o.z }, df[3] = { d.x, d.y, d.z };
    float uv[2], st[2], tx[3];
    tr_barycentrics(s->tri_verts + (size_t)id * 9, of, df, uv);
    tr_coordinate(X->uv6 + (size_t)id * 6, uv[0], uv[1], st);
    tr_lookup(T, st[0], st[1], tx);
    for (int k = 0; k < 3; ++k) out[k] = albedo[k] * tx[k];
    return 1;
}

/* ------------------------------------------------------------------------------------------------ §11 map (as tests/env_ref/) */
static void decode(float u, float v, float out[3])
{
    const float z = (1.0f - fabsf(u)) - fabsf(v);
    float x = u, y = v;
    if (z < 0.0f) { x = (1.0f - fabsf(v)) * sgn(u); y = (1.0f - fabsf(u)) * sgn(v); }
    const v3 d = norm3(mk(x, y, z));
    out[0] = d.x; out[1] = d.y; out[2] = d.z;
}

static uint32_t cell(float u, uint32_t n)
{
    int i = (int)floorf(fma_(u, 0.5f, 0.5f) * (float)n);
    if (i < 0) i = 0;
    if (i > (int)n - 1) i = (int)n - 1;
    return (uint32_t)i;
}

static float encode(const float d[3], uint32_t n, uint32_t ij[2])
{
    const float s = (fabsf(d[0]) + fabsf(d[1])) + fabsf(d[2]), is = 1.0f / s, px = d[0] * is, py = d[1] * is;
    float u = px, v = py;
    if (d[2] < 0.0f) { u = (1.0f - fabsf(py)) * sgn(px); v = (1.0f - fabsf(px)) * sgn(py); }
    ij[0] = cell(u, n); ij[1] = cell(v, n);
    return s;
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

static int env_table(const float *rgb, uint32_t n, float *texels4, float *mcdf, float *ccdf)
{
    const size_t nn = (size_t)n * n;
    double *w = malloc(sizeof(double) * nn), *R = malloc(sizeof(double) * n), total = 0.0;
    if (!w || !R) { free(w); free(R); return -1; }
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
        mcdf[j] = (lit && j + 1 < n) ? (float)(S / total) : 1.0f;
        double run = 0.0;
        for (uint32_t i = 0; i < n; ++i) {
            const size_t k = (size_t)j * n + i;
            run += w[k];
            ccdf[k] = (lit && R[j] > 0.0 && i + 1 < n) ? (float)(run / R[j]) : 1.0f;
            texels4[k * 4 + 0] = rgb[k * 3 + 0]; texels4[k * 4 + 1] = rgb[k * 3 + 1]; texels4[k * 4 + 2] = rgb[k * 3 + 2];
            texels4[k * 4 + 3] = lit ? (float)(w[k] / total * scale) : 0.0f;
        }
    }
    free(w); free(R);
    return lit;
}

typedef struct { uint32_t n, lit; float nf, step; float *tex, *mcdf, *ccdf; } env_t;

/* ------------------------------------------------------------------------------------------------ §7 light table (as tests/nee_ref/) */
typedef struct { v3 v0, e1, e2, nl; float area, pmf, pa; const float *le; } light_t;
typedef struct { uint32_t n; light_t *l; float *cdf; float *pa_of; } table_t;

static int build_table(const pto_scene *s, table_t *T)
{
    memset(T, 0, sizeof *T);
    const size_t cap = s->n_tris ? s->n_tris : 1;
    T->l = calloc(cap, sizeof(light_t)); T->cdf = calloc(cap, sizeof(float)); T->pa_of = calloc(cap, sizeof(float));
    double *w = calloc(cap, sizeof(double)), total = 0.0;
    uint32_t *id = calloc(cap, sizeof(uint32_t));
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
        T->l[j].pa = T->l[j].pmf / T->l[j].area;
        T->pa_of[id[j]] = T->l[j].pa;
    }
    free(w); free(id);
    return 0;
}

static uint32_t pick(const float *cdf, float u)
{
    uint32_t i = 0;
    while (!(u < cdf[i])) ++i;
    return i;
}

static uint32_t closest(const pto_scene *s, v3 o, v3 d, float *t)
{
    pto_stats st;
    memset(&st, 0, sizeof st);
    const float of[3] = { o.x, o.y, o.z }, df[3] = { d.x, d.y, d.z };
    return pto_closest(s, of, df, t, &st);
}

static const float *env_lookup(const env_t *E, v3 d, float *pdf)
{
    const float df[3] = { d.x, d.y, d.z };
    uint32_t ij[2];
    const float s = encode(df, E->n, ij);
    const float *tx = E->tex + ((size_t)ij[1] * E->n + ij[0]) * 4;
    *pdf = tx[3] / ((s * s) * s);
    return tx;
}

static void trace_pixel(const pto_scene *s, const pto_params *p, uint32_t flags, const table_t *T, const env_t *E, const tr_textures *X,
                        uint32_t x, uint32_t y, float out[4], tr_stats *st)
{
    const uint32_t K = p->streams ? p->streams : 1u;
    const int env_light = (flags & TR_NEE) && E && E->lit, tri_light = (flags & TR_NEE) && T->n > 0;
    const int nee = env_light || tri_light;
    const float psel = (env_light && tri_light) ? 0.5f : 1.0f;
    float accs[MAX_STREAMS][4];
    memset(accs, 0, sizeof accs);
    const uint32_t pixel = y * p->width + x;
    for (uint32_t si = 0; si < p->spp; ++si) {
        float *acc = accs[(p->sample_offset + si) % K];
        const uint32_t key = pto_path_key(p->seed, pixel, p->sample_offset + si);
        float of[3], df[3];
        pto_camera_ray((const pto_camera *)&s->cam, x, y, key, of, df);
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
                    for (int k = 0; k < 3; ++k) acc[k] = fma_(Tp[k], s->sky[k], acc[k]);
                } else {
                    float pdf, w = 1.0f;
                    const float *tx = env_lookup(E, d, &pdf);
                    if (env_light && pb_prev > 0.0f) {
                        const float pl = psel * pdf, q = pl / pb_prev;
                        w = nan0(1.0f / fma_(q, q, 1.0f));
                    }
                    for (int k = 0; k < 3; ++k) { const float e = tx[k] * w; acc[k] = fma_(Tp[k], e, acc[k]); }
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
            /* §13: the material this vertex shades with — the scene's, its albedo multiplied by the texel at a bound triangle's hit */
            pto_material me = s->mats[mat];
            if (id < s->n_tris) effective_albedo(s, X, id, o, d, s->mats[mat].albedo, me.albedo);
            const pto_material *m = &me;
            if (m->emission[0] != 0.0f || m->emission[1] != 0.0f || m->emission[2] != 0.0f) {
                float w = 1.0f;
                if (tri_light && pb_prev > 0.0f && id < s->n_tris && T->pa_of[id] > 0.0f) {
                    const float pl = ((T->pa_of[id] * psel) * (t * t)) / fabsf(dot3(ng, d)), q = pl / pb_prev;
                    w = nan0(1.0f / fma_(q, q, 1.0f));
                }
                for (int k = 0; k < 3; ++k) { const float e = m->emission[k] * w; acc[k] = fma_(Tp[k], e, acc[k]); }
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
                if (env_light && tri_light) {
                    env_branch = uc < 0.5f;
                    uc = env_branch ? uc * 2.0f : fma_(uc, 2.0f, -1.0f);
                }
                const v3 so = madd3(p->ray_eps, n, P);
                int traced = 0;
                v3 sd = mk(0, 0, 0);
                float f = 0.0f, tmax = 0.0f;
                const float *le = NULL;
                if (env_branch) {
                    const uint32_t j = pick(E->mcdf, uc), i = pick(E->ccdf + (size_t)j * E->n, pto_u01(key, 1025 + 3 * b));
                    const float u = fma_((float)i + pto_u01(key, 1026 + 3 * b), E->step, -1.0f);
                    const float v = fma_((float)j + pto_u01(key, 2048 + b), E->step, -1.0f);
                    float wl[3];
                    decode(u, v, wl);
                    sd = ld3(wl);
                    float pdf;
                    const float *tx = env_lookup(E, sd, &pdf);
                    const float cs = dot3(n, sd), pl = psel * pdf;
                    if (cs > 0.0f && pl > 0.0f) {
                        const float q = (cs * INV_PI) / pl;
                        f = nan0(q / fma_(q, q, 1.0f));
                        traced = 1; tmax = INFINITY; le = tx;
                    }
                } else {
                    const light_t *L = &T->l[pick(T->cdf, uc)];
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
                if (traced) {
                    float ts;
                    const uint32_t hid = closest(s, so, sd, &ts);
                    st->shadow_rays++;
                    if (hid == PTO_MISS || !(ts <= tmax))
                        for (int k = 0; k < 3; ++k) acc[k] = acc[k] + ((Tp[k] * W[k]) * f) * le[k]; /* W: the effective albedo */
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
    }
    const float is = 1.0f / (float)p->spp;
    for (int k = 0; k < 4; ++k) {
        float tot = accs[0][k];
        for (uint32_t j = 1; j < K; ++j) tot = tot + accs[j][k];
        out[k] = tot * is;
    }
}

/* env_rgb (may be NULL): env_n * env_n * 3 floats; X (may be NULL): the scene's textures. rgba: H*W*4 floats. */
int tr_render(const pto_scene *s, const pto_params *p, const float *env_rgb, uint32_t env_n, uint32_t flags, const tr_textures *X, int threads,
              float *rgba, tr_stats *st)
{
    if (!s || !p || !rgba || !st || p->spp == 0 || p->streams > MAX_STREAMS || (env_rgb && env_n == 0)) return -1;
    table_t T;
    if (build_table(s, &T) != 0) return -2;
    env_t E;
    memset(&E, 0, sizeof E);
    if (env_rgb) {
        const size_t nn = (size_t)env_n * env_n;
        E.n = env_n; E.nf = (float)env_n; E.step = 2.0f / (float)env_n;
        E.tex = malloc(sizeof(float) * 4 * nn); E.mcdf = malloc(sizeof(float) * env_n); E.ccdf = malloc(sizeof(float) * nn);
        if (!E.tex || !E.mcdf || !E.ccdf) return -2;
        const int lit = env_table(env_rgb, env_n, E.tex, E.mcdf, E.ccdf);
        if (lit < 0) return -2;
        E.lit = (uint32_t)lit;
    }
    memset(st, 0, sizeof *st);
    st->n_lights = T.n; st->lit = E.lit;
#ifdef _OPENMP
    if (threads > 0) omp_set_num_threads(threads);
#else
    (void)threads;
#endif
    uint64_t ext = 0, shadow = 0, paths = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : ext, shadow, paths)
    for (int y = 0; y < (int)p->height; ++y) {
        tr_stats loc;
        memset(&loc, 0, sizeof loc);
        for (uint32_t x = 0; x < p->width; ++x) {
            const size_t px = (size_t)y * p->width + x;
            trace_pixel(s, p, flags, &T, env_rgb ? &E : NULL, X, x, (uint32_t)y, rgba + px * 4, &loc);
        }
        ext += loc.ext_rays; shadow += loc.shadow_rays; paths += loc.paths;
    }
    st->ext_rays = ext; st->shadow_rays = shadow; st->paths = paths;
    free(T.l); free(T.cdf); free(T.pa_of); free(E.tex); free(E.mcdf); free(E.ccdf);
    return 0;
}
