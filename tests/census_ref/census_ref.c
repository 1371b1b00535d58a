/*
 * census_ref.c — TEST INFRASTRUCTURE ONLY: a scalar walker of docs/SPEC.md §5 that counts, per frame, how many path vertices fall in
 * each branch class of the BSDFs and of the path loop. The pieces of §2-§5 come from the oracle (oracle/pt_oracle.h): the camera ray,
 * the closest hit, the BSDF sample and the RNG; the loop around them is written here from §5. cr_render() must equal pto_render bit
 * for bit (frame, rays, paths), so its counts describe the very paths the oracle — and the device, held to the oracle — runs.
 * Nothing in the product may include, link or call this.
 *
 * Classes inside pto_bsdf_sample are told apart from its outputs (alive, side) and from float32 restatements of §5's conditions in
 * §5's expression order (al == 0, lensq > 0, sin2t >= 1, u3 < F). Where a restated condition and the sampler's output disagree
 * (a reflection although the restatement refracts, ...) the vertex is counted in CR_INCONSISTENT, which the tests require to be 0.
 */
#include <math.h>
#include <stdint.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif
#include "../../oracle/pt_oracle.h"

enum {
    CR_L_FRONT, CR_L_BACK, CR_M_MIRROR, CR_M_ROUGH, CR_M_ROUGH_DEAD, CR_M_ROUGH_NORMAL,
    CR_D_REFLECT_FRONT, CR_D_REFLECT_BACK, CR_D_REFRACT_FRONT, CR_D_REFRACT_BACK, CR_D_TIR_FRONT, CR_D_TIR_BACK, CR_D_ON_TRIANGLE,
    CR_T_BLACK, CR_RR_KILL, CR_RR_SURVIVE_CLAMPED, CR_RR_SURVIVE_UNCLAMPED, CR_DEPTH_CUT,
    CR_EMIT_METAL, CR_EMIT_DIELECTRIC, CR_EMIT_SPHERE, CR_MISS,
    CR_INCONSISTENT, /* not a class: restatement and sampler disagree (must stay 0) */
    CR_N
};
#define MAX_STREAMS 64
typedef struct { uint64_t rays, paths; uint64_t n[CR_N]; } cr_stats;

typedef struct { float x, y, z; } v3;
static inline v3 mk(float x, float y, float z) { v3 r = { x, y, z }; return r; }
static inline float fma_(float a, float b, float c) { return fmaf(a, b, c); }
static inline float min_(float a, float b) { return a < b ? a : b; }
static inline float max_(float a, float b) { return a > b ? a : b; }
static inline float dot3(v3 a, v3 b) { return fma_(a.z, b.z, fma_(a.y, b.y, a.x * b.x)); }
static inline v3 cross3(v3 a, v3 b) { return mk(fma_(a.y, b.z, -(a.z * b.y)), fma_(a.z, b.x, -(a.x * b.z)), fma_(a.x, b.y, -(a.y * b.x))); }
static inline v3 sub3(v3 a, v3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
static inline v3 madd3(float t, v3 d, v3 o) { return mk(fma_(t, d.x, o.x), fma_(t, d.y, o.y), fma_(t, d.z, o.z)); }
static inline v3 ld3(const float *p) { return mk(p[0], p[1], p[2]); }
static inline v3 norm3(v3 v) { float s = 1.0f / sqrtf(dot3(v, v)); return mk(v.x * s, v.y * s, v.z * s); }

/* §5 METAL, roughness al > 0: lensq of the stretched view vector (0 only at exact normal incidence) */
static float metal_lensq(float al, v3 d, v3 n)
{
    const float sg = copysignf(1.0f, n.z), a = -1.0f / (sg + n.z), b = n.x * n.y * a;
    const v3 tx = mk(fma_(sg * n.x, n.x * a, 1.0f), sg * b, -(sg * n.x)), ty = mk(b, fma_(n.y, n.y * a, sg), -n.y);
    const v3 wo = mk(-d.x, -d.y, -d.z);
    const v3 wl = mk(dot3(wo, tx), dot3(wo, ty), dot3(wo, n));
    const v3 Vh = norm3(mk(al * wl.x, al * wl.y, wl.z));
    return fma_(Vh.y, Vh.y, Vh.x * Vh.x);
}

/* §5 DIELECTRIC: 2 = total internal reflection (sin2t >= 1), 1 = Fresnel reflection (u3 < F), 0 = refraction */
static int dielectric_branch(float ior, v3 d, v3 n, int front, float u3)
{
    const float cosi = min_(max_(-dot3(d, n), 0.0f), 1.0f);
    const float eta = front ? 1.0f / ior : ior;
    const float sin2t = eta * eta * (1.0f - cosi * cosi);
    if (sin2t >= 1.0f) return 2;
    const float cost = sqrtf(1.0f - sin2t);
    const float ni = front ? 1.0f : ior, nt = front ? ior : 1.0f;
    const float rp = (nt * cosi - ni * cost) / (nt * cosi + ni * cost);
    const float rs = (ni * cosi - nt * cost) / (ni * cosi + nt * cost);
    const float F = 0.5f * (rp * rp + rs * rs);
    return u3 < F ? 1 : 0;
}

static void walk_pixel(const pto_scene *s, const pto_params *p, uint32_t x, uint32_t y, float out[4], cr_stats *st)
{
    const uint32_t K = p->streams ? p->streams : 1u;
    float accs[MAX_STREAMS][4];
    memset(accs, 0, sizeof accs);
    const uint32_t pixel = y * p->width + x;
    for (uint32_t si = 0; si < p->spp; ++si) {
        float *acc = accs[(p->sample_offset + si) % K];
        const uint32_t key = pto_path_key(p->seed, pixel, p->sample_offset + si);
        float of[3], df[3];
        pto_camera_ray(&s->cam, x, y, key, of, df);
        v3 o = ld3(of), d = ld3(df);
        float T[3] = { 1.0f, 1.0f, 1.0f };
        uint32_t depth = 0;
        for (;;) {
            float t;
            pto_stats ps;
            memset(&ps, 0, sizeof ps);
            const float oo[3] = { o.x, o.y, o.z }, dd[3] = { d.x, d.y, d.z };
            const uint32_t id = pto_closest(s, oo, dd, &t, &ps);
            st->rays++;
            depth++;
            if (id == PTO_MISS) {
                for (int k = 0; k < 3; ++k) acc[k] = fma_(T[k], s->sky[k], acc[k]);
                st->n[CR_MISS]++;
                break;
            }
            const v3 P = madd3(t, d, o);
            const int on_sphere = id >= s->n_tris;
            v3 ng;
            uint32_t mat;
            if (on_sphere) {
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
                for (int k = 0; k < 3; ++k) acc[k] = fma_(T[k], m->emission[k], acc[k]);
                if (m->kind == PTO_METAL) st->n[CR_EMIT_METAL]++;
                if (m->kind == PTO_DIELECTRIC) st->n[CR_EMIT_DIELECTRIC]++;
                if (on_sphere) st->n[CR_EMIT_SPHERE]++;
            }
            if (depth >= p->max_depth) { st->n[CR_DEPTH_CUT]++; break; }
            const uint32_t b = depth - 1;
            const float u1 = pto_u01(key, 4 + 4 * b), u2 = pto_u01(key, 5 + 4 * b), u3 = pto_u01(key, 6 + 4 * b);
            const float nv[3] = { n.x, n.y, n.z };
            float wi[3], W[3], side;
            const int alive = pto_bsdf_sample(m, dd, nv, front, u1, u2, u3, wi, W, &side);
            if (m->kind == PTO_LAMBERT) {
                st->n[front ? CR_L_FRONT : CR_L_BACK]++;
                if (!alive || side != 1.0f) st->n[CR_INCONSISTENT]++;
            } else if (m->kind == PTO_METAL) {
                if (m->roughness == 0.0f) {
                    st->n[CR_M_MIRROR]++;
                    if (!alive) st->n[CR_INCONSISTENT]++;
                } else {
                    st->n[alive ? CR_M_ROUGH : CR_M_ROUGH_DEAD]++;
                    if (!(metal_lensq(m->roughness, d, n) > 0.0f)) st->n[CR_M_ROUGH_NORMAL]++;
                }
                if (alive && side != 1.0f) st->n[CR_INCONSISTENT]++;
            } else {
                const int br = dielectric_branch(m->ior, d, n, front, u3);
                if (br == 2) st->n[front ? CR_D_TIR_FRONT : CR_D_TIR_BACK]++;
                else if (br == 1) st->n[front ? CR_D_REFLECT_FRONT : CR_D_REFLECT_BACK]++;
                else st->n[front ? CR_D_REFRACT_FRONT : CR_D_REFRACT_BACK]++;
                if (!on_sphere) st->n[CR_D_ON_TRIANGLE]++;
                if (!alive || side != (br == 0 ? -1.0f : 1.0f)) st->n[CR_INCONSISTENT]++;
            }
            if (!alive) break;
            for (int k = 0; k < 3; ++k) T[k] = T[k] * W[k];
            if (!(max_(T[0], max_(T[1], T[2])) > 0.0f)) { st->n[CR_T_BLACK]++; break; }
            if (depth >= p->rr_start) {
                const float qrr = min_(max_(T[0], max_(T[1], T[2])), 0.95f);
                if (!(pto_u01(key, 7 + 4 * b) < qrr)) { st->n[CR_RR_KILL]++; break; }
                st->n[qrr == 0.95f ? CR_RR_SURVIVE_CLAMPED : CR_RR_SURVIVE_UNCLAMPED]++;
                const float iq = 1.0f / qrr;
                for (int k = 0; k < 3; ++k) T[k] = T[k] * iq;
            }
            o = madd3(side * p->ray_eps, n, P);
            d = ld3(wi);
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

int cr_num_classes(void) { return CR_N; }

/* rgba: H*W*4 floats. st->n[c]: vertices (or path ends) of class c over the whole frame */
int cr_render(const pto_scene *s, const pto_params *p, int threads, float *rgba, cr_stats *st)
{
    if (!s || !p || !rgba || !st || p->spp == 0 || p->streams > MAX_STREAMS) return -1;
    memset(st, 0, sizeof *st);
#ifdef _OPENMP
    if (threads > 0) omp_set_num_threads(threads);
#else
    (void)threads;
#endif
#pragma omp parallel
    {
        cr_stats loc;
        memset(&loc, 0, sizeof loc);
#pragma omp for schedule(dynamic, 1)
        for (int y = 0; y < (int)p->height; ++y)
            for (uint32_t x = 0; x < p->width; ++x)
                walk_pixel(s, p, x, (uint32_t)y, rgba + ((size_t)y * p->width + x) * 4, &loc);
#pragma omp critical
        {
            st->rays += loc.rays; st->paths += loc.paths;
            for (int c = 0; c < CR_N; ++c) st->n[c] += loc.n[c];
        }
    }
    return 0;
}
