/*
 * motion_ref.c — TEST INFRASTRUCTURE ONLY: a scalar restatement of docs/SPEC.md §9 with §9.1 (pt_denoise_temporal with
 * PT_TEMPORAL_MOTION), written from the spec, one pixel after the other, independently of pathtracing_amd/ and of tests/temporal_ref/.
 * The camera rays come from the oracle (oracle/pt_oracle.h pto_camera_ray), the guides from tests/denoise_ref/ (§8.1). Nothing in the
 * product may include, link or call this.
 *
 * The history and the snapshot are the caller's: mr_accumulate() takes the frame, this call's guides and camera, the scene's current
 * triangles and spheres, and the previous call's guides, accumulated colour with lengths, camera and — if that call left one that this
 * call may use — its snapshot of the triangles and spheres. Whether a snapshot belongs to this scene (§9.1: same scene object, no commit
 * since) is the caller's to decide: it passes the snapshot or NULL. `variant` selects the spec as written or a deliberately wrong version
 * of §9.1 (MRV_*): the negative controls of tests/test_temporal_motion.py.
 */
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "../../oracle/pt_oracle.h"

/* pt_temporal_params (include/ptrt.h), 32 B */
typedef struct { uint32_t max_history; float plane_tolerance, normal_min; uint32_t flags; uint32_t pad[4]; } mr_params;
enum { MR_RESET = 1u, MR_MATCH_IDS = 2u, MR_MOTION = 8u };

/* §9 defaults, as exact f32 values */
#define MR_MAX_HISTORY 32u
#define MR_MAX_HISTORY_LIMIT 1048576u
#define MR_TAU_P 0x1p-7f
#define MR_TAU_N 0.875f

#define MISS 0xFFFFFFFFu

/* Wrong variants, for the negative controls only (0: the spec as written): the moved point is the new point (Pm = P); the taps are tested
 * against the new surface (P, n_p) although they were found through Pm; a moved triangle keeps n_p instead of nm; a moved sphere's offset
 * is not scaled by r'/r. */
enum { MRV_SPEC = 0, MRV_IGNORE_MOTION = 1, MRV_NEW_PLANE = 2, MRV_NEW_NORMAL = 3, MRV_NO_RADIUS_RATIO = 4 };

static inline float dot3(const float *a, const float *b) { return fmaf(a[2], b[2], fmaf(a[1], b[1], a[0] * b[0])); }
static inline void cross3(const float *a, const float *b, float *o)
{
    o[0] = fmaf(a[1], b[2], -(a[2] * b[1])); o[1] = fmaf(a[2], b[0], -(a[0] * b[2])); o[2] = fmaf(a[0], b[1], -(a[1] * b[0]));
}
static inline void sub3(const float *a, const float *b, float *o) { o[0] = a[0] - b[0]; o[1] = a[1] - b[1]; o[2] = a[2] - b[2]; }
static inline uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline int differ3(const float *a, const float *b) { return bits(a[0]) != bits(b[0]) || bits(a[1]) != bits(b[1]) || bits(a[2]) != bits(b[2]); }

/* the parameters with their defaults filled in; 0, or -1 for refused parameters (bit 4 is unassigned) */
int mr_resolve(const mr_params *in, mr_params *out)
{
    *out = *in;
    if (in->flags & ~(MR_RESET | MR_MATCH_IDS | MR_MOTION)) return -1;
    if (in->max_history > MR_MAX_HISTORY_LIMIT) return -1;
    if (!(in->plane_tolerance >= 0.0f) || isinf(in->plane_tolerance)) return -1;
    if (!(in->normal_min >= 0.0f && in->normal_min <= 1.0f)) return -1;
    if (!out->max_history) out->max_history = MR_MAX_HISTORY;
    if (out->plane_tolerance == 0.0f) out->plane_tolerance = MR_TAU_P;
    if (out->normal_min == 0.0f) out->normal_min = MR_TAU_N;
    return 0;
}

typedef struct { float sw, sc[3], sl; } sums;

/* what is the same for every pixel of a call */
typedef struct {
    uint32_t W, H;
    const float *old_g8, *old_h;
    pto_camera oc;           /* cam', jitter off */
    float tp2, tau_n;
    int match;
} call;

/* one tap of §9 / §9.1: old pixel (qx, qy) with weight bw, tested against the point Pt and the normal nt */
static void tap(const call *c, int qx, int qy, float bw, const float *Pt, const float *nt, uint32_t id, float e2, sums *s)
{
    if (qx < 0 || qy < 0 || qx >= (int)c->W || qy >= (int)c->H) return;
    const size_t iq = (size_t)qy * c->W + (size_t)qx;
    const float *gq = c->old_g8 + iq * 8, *hq = c->old_h + iq * 4;
    if (bits(gq[7]) == MISS) return;
    float o2[3], d2[3];
    pto_camera_ray(&c->oc, (uint32_t)qx, (uint32_t)qy, 0u, o2, d2);
    const float P2[3] = { fmaf(gq[3], d2[0], o2[0]), fmaf(gq[3], d2[1], o2[1]), fmaf(gq[3], d2[2], o2[2]) };
    float dP[3];
    sub3(P2, Pt, dP);
    const float k = dot3(dP, nt);
    if (!(k * k <= c->tp2 * e2)) return;
    if (!(dot3(nt, gq) >= c->tau_n)) return;
    if (c->match && bits(gq[7]) != id) return;
    s->sw = s->sw + bw;
    for (int k3 = 0; k3 < 3; ++k3) s->sc[k3] = fmaf(bw, hq[k3], s->sc[k3]);
    s->sl = fmaf(bw, hq[3], s->sl);
}

/*
 * §9 + §9.1 for one call. frame: W*H*4; g8: W*H*8 (§8.1 of this call); cam: the scene's camera. tris: NT*9 current vertices by original
 * id (the device record of §4.3 is v0, v1 - v0, v2 - v0 of these); sph: NS*4. History: old_g8, old_h (W*H*4: accumulated rgb | length) and
 * old_cam of the previous call, of the same size — old_cam == NULL: no history. snap_tris / snap_sph: the snapshot this call may use (both
 * NULL: none; it is used only with MR_MOTION and a history). out: W*H*4 accumulated rgb | frame alpha; new_h: W*H*4 accumulated rgb |
 * length; reproj (may be NULL): W*H*3 = (fx, fy, valid) as in tests/temporal_ref/; moved_mask (may be NULL): W*H bytes, 1 where the pixel's
 * primitive counted as moved; n_moved (may be NULL): their number. Returns the number of pixels with l > 1, or -1 for refused parameters.
 */
long mr_accumulate(const float *frame, const float *g8, const pto_camera *cam, uint32_t W, uint32_t H, const float *tris, uint32_t NT,
                   const float *sph, uint32_t NS, const float *old_g8, const float *old_h, const pto_camera *old_cam,
                   const float *snap_tris, const float *snap_sph, const mr_params *params, int variant, float *out, float *new_h,
                   float *reproj, uint8_t *moved_mask, long *n_moved)
{
    mr_params p;
    if (mr_resolve(params, &p) < 0) return -1;
    const int history = old_cam && old_g8 && old_h && !(p.flags & MR_RESET) && p.max_history != 1u;
    const int uses = history && (p.flags & MR_MOTION) && (snap_tris || !NT) && (snap_sph || !NS) && (snap_tris || snap_sph);
    pto_camera c0 = *cam;
    call c;
    c.W = W; c.H = H; c.old_g8 = old_g8; c.old_h = old_h;
    c.oc = history ? *old_cam : *cam;
    const int same = memcmp(&c0, &c.oc, sizeof c0) == 0; /* the 16 words, jitter included */
    c0.jitter = 0u; c.oc.jitter = 0u;
    c.tp2 = p.plane_tolerance * p.plane_tolerance; c.tau_n = p.normal_min;
    c.match = (p.flags & MR_MATCH_IDS) != 0;
    const float maxl = (float)p.max_history;
    float A[3], B[3], Cx[3];
    cross3(c.oc.right, c.oc.up, A); cross3(c.oc.up, c.oc.forward, B); cross3(c.oc.forward, c.oc.right, Cx);
    const float det = dot3(c.oc.forward, A);
    long taken = 0, moved_total = 0;
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            const size_t ip = (size_t)y * W + x;
            const float *cp = frame + ip * 4, *g = g8 + ip * 8;
            float *o = out + ip * 4, *nh = new_h + ip * 4;
            float l = 1.0f;
            int moved = 0;
            o[0] = cp[0]; o[1] = cp[1]; o[2] = cp[2]; o[3] = cp[3];
            if (reproj) { reproj[ip * 3] = reproj[ip * 3 + 1] = reproj[ip * 3 + 2] = 0.0f; }
            const uint32_t id = bits(g[7]);
            if (history && id != MISS) {
                float ro[3], rd[3];
                pto_camera_ray(&c0, x, y, 0u, ro, rd);
                const float P[3] = { fmaf(g[3], rd[0], ro[0]), fmaf(g[3], rd[1], ro[1]), fmaf(g[3], rd[2], ro[2]) };
                float Pm[3] = { P[0], P[1], P[2] }, nm[3] = { g[0], g[1], g[2] }; /* an unmoved pixel: §9's P, n_p */
                float wv[3];
                sub3(P, c.oc.origin, wv);
                if (uses && id < NT) {
                    const float *v = tris + (size_t)id * 9, *sv = snap_tris + (size_t)id * 9;
                    float e1[3], e2v[3], e1s[3], e2s[3];
                    sub3(v + 3, v, e1); sub3(v + 6, v, e2v);       /* the current device record: v0, e1, e2 */
                    sub3(sv + 3, sv, e1s); sub3(sv + 6, sv, e2s);   /* the snapshot's */
                    moved = differ3(sv, v) || differ3(e1s, e1) || differ3(e2s, e2v);
                    if (moved) {
                        float pp[3], tv[3], qq[3], ng[3], cr[3];
                        cross3(rd, e2v, pp);
                        const float dt = dot3(e1, pp), inv_det = 1.0f / dt;
                        sub3(ro, v, tv);
                        const float u = dot3(tv, pp) * inv_det;
                        cross3(tv, e1, qq);
                        const float vv = dot3(rd, qq) * inv_det;
                        if (variant != MRV_IGNORE_MOTION)
                            for (int k = 0; k < 3; ++k) Pm[k] = fmaf(vv, e2s[k], fmaf(u, e1s[k], sv[k]));
                        cross3(e1s, e2s, cr);
                        const float s = 1.0f / sqrtf(dot3(cr, cr));
                        ng[0] = cr[0] * s; ng[1] = cr[1] * s; ng[2] = cr[2] * s;
                        sub3(Pm, c.oc.origin, wv);
                        const int front = dot3(ng, wv) < 0.0f;
                        if (variant != MRV_NEW_NORMAL)
                            for (int k = 0; k < 3; ++k) nm[k] = front ? ng[k] : -ng[k];
                    }
                } else if (uses && id - NT < NS) {
                    const float *s4 = sph + (size_t)(id - NT) * 4, *ss = snap_sph + (size_t)(id - NT) * 4;
                    moved = differ3(ss, s4) || bits(ss[3]) != bits(s4[3]);
                    if (moved) {
                        const float s = variant == MRV_NO_RADIUS_RATIO ? 1.0f : ss[3] / s4[3];
                        if (variant != MRV_IGNORE_MOTION)
                            for (int k = 0; k < 3; ++k) Pm[k] = fmaf(P[k] - s4[k], s, ss[k]);
                        sub3(Pm, c.oc.origin, wv);
                    }
                }
                const float e2 = dot3(wv, wv);
                /* what the taps are tested against: the surface as it was */
                const float *Pt = variant == MRV_NEW_PLANE ? P : Pm, *nt = variant == MRV_NEW_PLANE ? g : nm;
                sums s = { 0.0f, { 0.0f, 0.0f, 0.0f }, 0.0f };
                if (same && !moved) {
                    if (reproj) { reproj[ip * 3] = (float)x; reproj[ip * 3 + 1] = (float)y; reproj[ip * 3 + 2] = 1.0f; }
                    tap(&c, (int)x, (int)y, 1.0f, Pt, nt, id, e2, &s);
                } else {
                    const float den = dot3(wv, A);
                    if ((den > 0.0f && det > 0.0f) || (den < 0.0f && det < 0.0f)) {
                        const float inv = 1.0f / den;
                        const float sx = dot3(wv, B) * inv, sy = dot3(wv, Cx) * inv;
                        const float fx = (sx + c.oc.cx) / c.oc.scale - 0.5f, fy = (sy + c.oc.cy) / c.oc.scale - 0.5f;
                        if (fx >= -1.0f && fx < (float)W && fy >= -1.0f && fy < (float)H) {
                            if (reproj) { reproj[ip * 3] = fx; reproj[ip * 3 + 1] = fy; reproj[ip * 3 + 2] = 1.0f; }
                            const float x0 = floorf(fx), y0 = floorf(fy), bx = fx - x0, by = fy - y0;
                            for (int j = 0; j < 2; ++j)
                                for (int i = 0; i < 2; ++i)
                                    tap(&c, (int)x0 + i, (int)y0 + j, (i ? bx : 1.0f - bx) * (j ? by : 1.0f - by), Pt, nt, id, e2, &s);
                        }
                    }
                }
                if (s.sw >= 0.25f) {
                    const float r = 1.0f / s.sw;
                    l = fminf(s.sl * r + 1.0f, maxl);
                    const float a = 1.0f / l;
                    for (int k = 0; k < 3; ++k) { const float hk = s.sc[k] * r; o[k] = fmaf(a, cp[k] - hk, hk); }
                }
            }
            nh[0] = o[0]; nh[1] = o[1]; nh[2] = o[2]; nh[3] = l;
            taken += l > 1.0f;
            moved_total += moved;
            if (moved_mask) moved_mask[ip] = (uint8_t)moved;
        }
    if (n_moved) *n_moved = moved_total;
    return taken;
}
