/*
 * lens_ref.c — TEST INFRASTRUCTURE ONLY: a scalar restatement of docs/SPEC.md §3.1 (the thin-lens camera), written from the spec and
 * independently of pathtracing_amd/. §5's loop and §7's light sample are restated around the lens ray, as tests/nee_ref/nee_ref.c does
 * around the pinhole ray. The closest hit, the BSDF sample, the RNG and sincos2pi come from the oracle (oracle/pt_oracle.h). Nothing in
 * the product may include, link or call this.
 *
 * lr_render() with lens == NULL or radius 0 takes the oracle's pinhole ray: with flags = 0 it must equal pto_render, with LR_NEE
 * nr_render, bit for bit. It reports extension and shadow rays separately and, optionally, per-pixel sums of squared per-sample radiance.
 * LR_FOCUS_IGNORED, LR_LINEAR_RADIUS and LR_FIXED_ORIGIN are deliberate errors for the tests' negative controls.
 * A lens outside §3.1's domain (lr_lens_domain) is refused by lr_render and lr_camera_ray, as pt_render refuses it.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif
#include "../../oracle/pt_oracle.h"

enum { LR_NEE = 1, LR_FOCUS_IGNORED = 2, LR_LINEAR_RADIUS = 4, LR_FIXED_ORIGIN = 8 };
typedef struct { float radius, focus_distance; } lr_lens;
typedef struct { uint64_t ext_rays, shadow_rays, paths, n_lights; } lr_stats;

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
#define INV_PI 0.318309873f
#define MAX_STREAMS 64

/* §3.1, once per frame: lens_u = R * right / |right|, lens_v = R * up / |up|. -1: a dot product is 0 or a component is not finite. */
int lr_lens_basis(const pto_camera *c, float R, float lens_u[3], float lens_v[3])
{
    const float dr = dot3(ld3(c->right), ld3(c->right)), du = dot3(ld3(c->up), ld3(c->up));
    if (dr == 0.0f || du == 0.0f) return -1;
    const float ru = R * (1.0f / sqrtf(dr)), rv = R * (1.0f / sqrtf(du));
    for (int k = 0; k < 3; ++k) {
        lens_u[k] = c->right[k] * ru;
        lens_v[k] = c->up[k] * rv;
        if (!isfinite(lens_u[k]) || !isfinite(lens_v[k])) return -1;
    }
    return 0;
}

/* The largest |pto_sincos2pi(u) - (sin, cos)(2 pi u)| in double (libm) over u = i * 2^-24, i = first, first + step, ... < end: what
 * tests/lens64.py's bound takes for the one function of §3.1 whose error §0 does not state. */
double lr_sincos2pi_error(uint32_t first, uint32_t end, uint32_t step)
{
    double worst = 0.0;
    for (uint64_t i = first; i < end; i += step ? step : 1u) {
        const float u = (float)i * 5.9604644775390625e-8f;
        float sn, cs;
        pto_sincos2pi(u, &sn, &cs);
        const double ang = 6.283185307179586476925286766559 * (double)u;
        worst = fmax(worst, fmax(fabs((double)sn - sin(ang)), fabs((double)cs - cos(ang))));
    }
    return worst;
}

/* §3.1 "Domain", from the section's text: 0 if a w x h frame of camera c through (R, F) is inside it, else -1. */
int lr_lens_domain(const pto_camera *c, float R, float F, uint32_t w, uint32_t h)
{
    double r[3], u[3], f[3], n[3], rr = 0.0, uu = 0.0, ru = 0.0, nn = 0.0, fn = 0.0;
    for (int k = 0; k < 3; ++k) { r[k] = c->right[k]; u[k] = c->up[k]; f[k] = c->forward[k]; }
    for (int k = 0; k < 3; ++k) {
        n[k] = r[(k + 1) % 3] * u[(k + 2) % 3] - r[(k + 2) % 3] * u[(k + 1) % 3];
        rr += r[k] * r[k]; uu += u[k] * u[k]; ru += r[k] * u[k];
    }
    for (int k = 0; k < 3; ++k) { nn += n[k] * n[k]; fn += f[k] * n[k]; }
    nn = sqrt(nn); rr = sqrt(rr); uu = sqrt(uu);
    if (!(nn > ldexp(rr * uu, -6))) return -1;
    const double sc = c->scale, cx = c->cx, cy = c->cy, tw = w * fabs(sc) + fabs(cx), th = h * fabs(sc) + fabs(cy);
    const double x0 = fmin(-cx, w * sc - cx) - ldexp(tw, -22), x1 = fmax(-cx, w * sc - cx) + ldexp(tw, -22);
    const double y0 = fmin(-cy, h * sc - cy) - ldexp(th, -22), y1 = fmax(-cy, h * sc - cy) + ldexp(th, -22);
    double vmax = 0.0, ff = 0.0;
    for (int i = 0; i < 4; ++i) {
        const double sx = (i & 1) ? x1 : x0, sy = (i & 2) ? y1 : y0;
        double l2 = 0.0;
        for (int k = 0; k < 3; ++k) { const double v = f[k] + sx * r[k] + sy * u[k]; l2 += v * v; }
        if (!isfinite(l2)) return -1;
        vmax = fmax(vmax, sqrt(l2));
    }
    for (int k = 0; k < 3; ++k) ff += f[k] * f[k];
    const double hi = (double)F * vmax + (double)R * sqrt(1.0 + fabs(ru) / (rr * uu));
    const double S = sqrt(ff) + (fmax(fabs(cx), fabs(w * sc - cx)) + tw) * rr + (fmax(fabs(cy), fabs(h * sc - cy)) + th) * uu;
    const double lo = (double)F * (fabs(fn) / nn - ldexp(S, -11));
    return (lo >= ldexp(1.0, -60) && hi * hi <= ldexp(1.0, 127)) ? 0 : -1;
}

/* §3.1: the camera ray of pixel (x, y) with `key` through the lens (lu, lv, F) */
static void lens_ray(const pto_camera *c, const float lu[3], const float lv[3], float F, uint32_t flags, uint32_t x, uint32_t y, uint32_t key,
                     float o[3], float d[3])
{
    const float jx = c->jitter ? pto_u01(key, 0) : 0.5f, jy = c->jitter ? pto_u01(key, 1) : 0.5f;
    const float sx = ((float)x + jx) * c->scale - c->cx, sy = ((float)y + jy) * c->scale - c->cy;
    float v[3], a[3], w[3];
    for (int k = 0; k < 3; ++k) v[k] = fma_(sy, c->up[k], fma_(sx, c->right[k], c->forward[k]));
    const float u = pto_u01(key, 2);
    const float r = (flags & LR_LINEAR_RADIUS) ? u : sqrtf(u);
    float sn, cs;
    pto_sincos2pi(pto_u01(key, 3), &sn, &cs);
    const float lx = r * cs, ly = r * sn;
    for (int k = 0; k < 3; ++k) {
        a[k] = fma_(ly, lv[k], lx * lu[k]);
        o[k] = (flags & LR_FIXED_ORIGIN) ? c->origin[k] : c->origin[k] + a[k];
        w[k] = (flags & LR_FOCUS_IGNORED) ? v[k] - a[k] : fma_(F, v[k], -a[k]);
    }
    const v3 n = norm3(ld3(w));
    d[0] = n.x; d[1] = n.y; d[2] = n.z;
}

/* 0, -1 for a degenerate basis (lr_lens_basis), or -2 for a lens outside §3.1's domain in a w x h frame (w == 0: the caller's frame was
 * accepted already, the rule is not asked) */
int lr_camera_ray(const pto_camera *c, const lr_lens *lens, uint32_t w, uint32_t h, uint32_t x, uint32_t y, uint32_t key, float o[3], float d[3])
{
    float lu[3], lv[3];
    if (w != 0u && lr_lens_domain(c, lens->radius, lens->focus_distance, w, h) != 0) return -2;
    if (lr_lens_basis(c, lens->radius, lu, lv) != 0) return -1;
    lens_ray(c, lu, lv, lens->focus_distance, 0u, x, y, key, o, d);
    return 0;
}

/* §7's light table, restated as nee_ref.c restates it */
typedef struct { v3 v0, e1, e2, nl; float area, pmf, pa; const float *le; } light_t;
typedef struct { uint32_t n; light_t *l; float *cdf; float *pa_of; } table_t;

static int build_table(const pto_scene *s, table_t *T)
{
    memset(T, 0, sizeof *T);
    const size_t cap = s->n_tris ? s->n_tris : 1;
    T->l = calloc(cap, sizeof(light_t));
    T->cdf = calloc(cap, sizeof(float));
    T->pa_of = calloc(cap, sizeof(float));
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

static uint32_t pick(const table_t *T, float u)
{
    uint32_t i = 0;
    while (!(u < T->cdf[i])) ++i;
    return i;
}

static uint32_t closest(const pto_scene *s, v3 o, v3 d, float *t)
{
    pto_stats st;
    memset(&st, 0, sizeof st);
    const float of[3] = { o.x, o.y, o.z }, df[3] = { d.x, d.y, d.z };
    return pto_closest(s, of, df, t, &st);
}

typedef struct { int on; float lu[3], lv[3], F; } lens_t;

static void trace_pixel(const pto_scene *s, const pto_params *p, const lens_t *ln, uint32_t flags, const table_t *T, uint32_t x, uint32_t y,
                        float out[4], double *sq, lr_stats *st)
{
    const uint32_t K = p->streams ? p->streams : 1u;
    const int nee = (flags & LR_NEE) && T->n > 0;
    float accs[MAX_STREAMS][4];
    memset(accs, 0, sizeof accs);
    const uint32_t pixel = y * p->width + x;
    for (uint32_t si = 0; si < p->spp; ++si) {
        float *acc = accs[(p->sample_offset + si) % K];
        float val[3] = { 0.0f, 0.0f, 0.0f };
        const uint32_t key = pto_path_key(p->seed, pixel, p->sample_offset + si);
        float of[3], df[3];
        if (ln->on) lens_ray(&s->cam, ln->lu, ln->lv, ln->F, flags, x, y, key, of, df);
        else pto_camera_ray(&s->cam, x, y, key, of, df);
        v3 o = ld3(of), d = ld3(df);
        float Tp[3] = { 1.0f, 1.0f, 1.0f };
        float pb_prev = 0.0f;
        uint32_t depth = 0;
        for (;;) { /* §5 from `hit = closest(o, d)` on, unchanged */
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
                float w = 1.0f;
                if (nee && pb_prev > 0.0f && id < s->n_tris && T->pa_of[id] > 0.0f) {
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
            if (nee && m->kind == PTO_LAMBERT) { /* §7 */
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
                    const float pl = (L->pa * dist2) / cl, q = (cs * INV_PI) / pl;
                    const float f = nan0(q / fma_(q, q, 1.0f));
                    const float tmax = dist * 0.9999f;
                    float ts;
                    const uint32_t hid = closest(s, so, sd, &ts);
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

/* lens (may be NULL; radius 0 = none): the scene's lens. rgba: H*W*4 floats; sq (may be NULL): H*W*3 doubles, per pixel and channel the
 * sum over samples of the squared sample radiance. -3: a degenerate basis (lr_lens_basis); -4: a lens outside §3.1's domain, checked first
 * as pt_render does. */
int lr_render(const pto_scene *s, const pto_params *p, const lr_lens *lens, uint32_t flags, int threads, float *rgba, double *sq, lr_stats *st)
{
    if (!s || !p || !rgba || !st || p->spp == 0 || p->streams > MAX_STREAMS) return -1;
    lens_t ln;
    memset(&ln, 0, sizeof ln);
    if (lens && lens->radius > 0.0f) {
        if (lr_lens_domain(&s->cam, lens->radius, lens->focus_distance, p->width, p->height) != 0) return -4;
        if (lr_lens_basis(&s->cam, lens->radius, ln.lu, ln.lv) != 0) return -3;
        ln.on = 1; ln.F = lens->focus_distance;
    }
    table_t T;
    if (build_table(s, &T) != 0) return -2;
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
        lr_stats loc;
        memset(&loc, 0, sizeof loc);
        for (uint32_t x = 0; x < p->width; ++x) {
            const size_t px = (size_t)y * p->width + x;
            trace_pixel(s, p, &ln, flags, &T, x, (uint32_t)y, rgba + px * 4, sq ? sq + px * 3 : NULL, &loc);
        }
        ext += loc.ext_rays; shadow += loc.shadow_rays; paths += loc.paths;
    }
    st->ext_rays = ext; st->shadow_rays = shadow; st->paths = paths;
    free(T.l); free(T.cdf); free(T.pa_of);
    return 0;
}
