// temporal.hip — pt_denoise_temporal (docs/SPEC.md §9) on gfx950: reprojection of the previous call's history and the blend with the
// assembled frame, one fused kernel per call.
//
//   k_temporal : 64x4 workgroups as k_atrous: a wave covers 64 pixels of one row, so the centre reads (frame, g0, g1) and the two stores
//                are one coalesced 1 KiB row each. A pixel rebuilds its world position from its own guide depth, projects it through the
//                history's camera and takes up to four bilinear taps of the old guides and the old accumulated colour (length in .w);
//                under smooth motion neighbouring lanes land on neighbouring old pixels. Pixels that took history are counted by
//                ballot, one atomic per wave, spread over kTemporalCounters counter lines that the host adds up.
//   k_temporal_motion : the same pass for a call that uses the geometry snapshot (§9.1, PT_TEMPORAL_MOTION): a pixel whose primitive's
//                device record differs from its snapshot finds where its surface point was at the previous call (the triangle's
//                barycentrics carried to the old vertices, a sphere's offset scaled to the old radius), projects that point through the
//                history's camera and tests the taps against the surface as it was. Three gathers per pixel (blob index, 64-B record,
//                36-B old vertices), which neighbouring pixels of one triangle share. Unmoved pixels run k_temporal's arithmetic.
// What the two share — the gather through the history's camera, the blend, the two stores, the counter line — is stated once, in the
// device functions ahead of them.
// Op order follows §9 and §9.1 exactly (explicit fma, -ffp-contract=off, IEEE division): tests/temporal_ref/ and tests/motion_ref/ restate
// them bit for bit. Includes pt_device.h for the vector helpers and §3's camera ray only.
#include "ptrt_internal.h"
#include "pt_device.h"
#include "temporal.h"
#include <cstring>

using namespace ptd;

namespace ptrt {

namespace {
struct TemporalKernelArgs { // TemporalArgs with the cameras in the device's own type
    Camera cam, old_cam;
    uint32_t width, height, has_history, same_camera, match_ids;
    float max_history, tau_p2, tau_n;
    const float4 *frame, *g0, *g1, *old_g0, *old_g1, *old_h;
    float4 *out, *new_h;
    uint32_t *taken;
};

struct TapSums { float sw, sr, sg, sb, sl; };

// One tap of §9: old pixel (qx, qy) with bilinear weight bw, tested against the plane and the normal of the new pixel
PT_DEV void temporal_tap(const TemporalKernelArgs &a, int qx, int qy, float bw, V3 P, V3 n, uint32_t id, float e2, TapSums &s)
{
    if (qx < 0 || qy < 0 || qx >= (int)a.width || qy >= (int)a.height) return;
    const size_t iq = (size_t)qy * a.width + (size_t)qx;
    const float4 aq = a.old_g1[iq];
    const uint32_t idq = __float_as_uint(aq.w);
    if (idq == PT_MISS) return;
    const float4 nq = a.old_g0[iq];
    V3 o2, d2;
    camera_ray(a.old_cam, (uint32_t)qx, (uint32_t)qy, 0u, o2, d2); // old_cam.jitter == 0
    const V3 P2 = madd(nq.w, d2, o2);
    const float k = dot(P2 - P, n);
    if (!(k * k <= a.tau_p2 * e2)) return;
    if (!(dot(n, xyz(nq)) >= a.tau_n)) return;
    if (a.match_ids && idq != id) return;
    const float4 hq = a.old_h[iq];
    s.sw = s.sw + bw;
    s.sr = fma_(bw, hq.x, s.sr); s.sg = fma_(bw, hq.y, s.sg); s.sb = fma_(bw, hq.z, s.sb);
    s.sl = fma_(bw, hq.w, s.sl);
}

// §9.1's extra inputs: the scene as it is and as the snapshot holds it
struct MotionKernelArgs {
    const uint32_t *blob_of;        // original triangle id -> blob index
    const float4 *tris, *spheres;   // DeviceScene's
    const float *snap_tris;         // 9 floats per triangle, by original id
    const float4 *snap_spheres;
    uint32_t n_tris, n_spheres;
    uint32_t *moved;                // counter lines like `taken`: hit pixels whose primitive moved
};

PT_DEV bool differs(float a, float b) { return __float_as_uint(a) != __float_as_uint(b); }
PT_DEV bool differs(V3 a, V3 b) { return differs(a.x, b.x) || differs(a.y, b.y) || differs(a.z, b.z); }

// §9's gather for pixel (x, y): surface point P with normal n and id, wv = P - the old camera's origin. `in_place`: P projects to the
// pixel itself, one tap there; otherwise P goes through the history's camera and up to four bilinear taps count
PT_DEV TapSums gather_history(const TemporalKernelArgs &a, uint32_t x, uint32_t y, bool in_place, V3 P, V3 n, V3 wv, uint32_t id)
{
    const float e2 = dot(wv, wv);
    TapSums s{ 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
    if (in_place) {
        temporal_tap(a, (int)x, (int)y, 1.0f, P, n, id, e2, s);
    } else {
        const V3 f2 = V3{ a.old_cam.forward[0], a.old_cam.forward[1], a.old_cam.forward[2] };
        const V3 r2 = V3{ a.old_cam.right[0], a.old_cam.right[1], a.old_cam.right[2] };
        const V3 u2 = V3{ a.old_cam.up[0], a.old_cam.up[1], a.old_cam.up[2] };
        const V3 A = cross(r2, u2), B = cross(u2, f2), Cx = cross(f2, r2);
        const float det = dot(f2, A), den = dot(wv, A);
        if ((den > 0.0f && det > 0.0f) || (den < 0.0f && det < 0.0f)) {
            const float inv = 1.0f / den;
            const float sx = dot(wv, B) * inv, sy = dot(wv, Cx) * inv;
            const float fx = (sx + a.old_cam.cx) / a.old_cam.scale - 0.5f;
            const float fy = (sy + a.old_cam.cy) / a.old_cam.scale - 0.5f;
            if (fx >= -1.0f && fx < (float)a.width && fy >= -1.0f && fy < (float)a.height) { // (a NaN ends here)
                const float x0 = __builtin_floorf(fx), y0 = __builtin_floorf(fy);
                const float bx = fx - x0, by = fy - y0;
                const int ix = (int)x0, iy = (int)y0;
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int i = 0; i < 2; ++i)
                        temporal_tap(a, ix + i, iy + j, (i ? bx : 1.0f - bx) * (j ? by : 1.0f - by), P, n, id, e2, s);
            }
        }
    }
    return s;
}

// §9's blend of the frame's colour c into what the taps gathered: the output colour and the new length l. Sums of too little weight
// (none: no history, a miss, no tap passed) give c and l = 1
PT_DEV float4 blend(const TemporalKernelArgs &a, float4 c, const TapSums &s, float &l)
{
    l = 1.0f;
    if (!(s.sw >= 0.25f)) return c;
    const float r = 1.0f / s.sw;
    const float hr = s.sr * r, hg = s.sg * r, hb = s.sb * r;
    l = fmin_(s.sl * r + 1.0f, a.max_history);
    const float w = 1.0f / l;
    return make_float4(fma_(w, c.x - hr, hr), fma_(w, c.y - hg, hg), fma_(w, c.z - hb, hb), c.w);
}

// The two stores of a pixel; true if it took history
PT_DEV bool store_pixel(const TemporalKernelArgs &a, size_t ip, float4 out, float l)
{
    a.out[ip] = out;
    a.new_h[ip] = make_float4(out.x, out.y, out.z, l);
    return l > 1.0f;
}

// A wave is one row segment (threadIdx.y); no lane has left when it counts by ballot, so lane 0 speaks for it. Consecutive waves add to
// consecutive counter lines: tens of thousands of atomics on one address would take longer than the rest of the kernel
// (ptrt_internal.h kShards). The first word of this wave's line
PT_DEV uint32_t counter_line()
{
    return (((blockIdx.y * gridDim.x + blockIdx.x) * 4u + threadIdx.y) % kTemporalCounters) * kCounterStride;
}
} // namespace

__global__ void __launch_bounds__(kBlock) k_temporal(TemporalKernelArgs a)
{
    const uint32_t x = blockIdx.x * 64u + threadIdx.x, y = blockIdx.y * 4u + threadIdx.y;
    bool took = false;
    if (x < a.width && y < a.height) {
        const size_t ip = (size_t)y * a.width + x;
        const float4 c = a.frame[ip];
        TapSums s{ 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
        if (a.has_history) { // uniform over the grid
            const float4 ap = a.g1[ip];
            const uint32_t id = __float_as_uint(ap.w);
            if (id != PT_MISS) {
                const float4 np = a.g0[ip];
                V3 o, d;
                camera_ray(a.cam, x, y, 0u, o, d); // cam.jitter == 0: §8.1's ray
                const V3 P = madd(np.w, d, o);
                const V3 wv = P - V3{ a.old_cam.origin[0], a.old_cam.origin[1], a.old_cam.origin[2] };
                s = gather_history(a, x, y, a.same_camera, P, xyz(np), wv, id);
            }
        }
        float l;
        const float4 out = blend(a, c, s, l);
        took = store_pixel(a, ip, out, l);
    }
    const unsigned long long m = __ballot(took);
    if (threadIdx.x == 0u && m) atomicAdd(a.taken + counter_line(), (uint32_t)__popcll(m));
}

__global__ void __launch_bounds__(kBlock) k_temporal_motion(TemporalKernelArgs a, MotionKernelArgs g)
{
    const uint32_t x = blockIdx.x * 64u + threadIdx.x, y = blockIdx.y * 4u + threadIdx.y;
    bool took = false, moved = false;
    if (x < a.width && y < a.height) {
        const size_t ip = (size_t)y * a.width + x;
        const float4 c = a.frame[ip];
        TapSums s{ 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
        const float4 ap = a.g1[ip];
        const uint32_t id = __float_as_uint(ap.w);
        if (id != PT_MISS) { // (a call that uses the snapshot has a history)
            const float4 np = a.g0[ip];
            V3 n = xyz(np);
            V3 o, d;
            camera_ray(a.cam, x, y, 0u, o, d); // cam.jitter == 0: §8.1's ray
            V3 P = madd(np.w, d, o);
            const V3 o2 = V3{ a.old_cam.origin[0], a.old_cam.origin[1], a.old_cam.origin[2] };
            V3 wv = P - o2;
            if (id < g.n_tris) {
                const float4 *rec = g.tris + (size_t)g.blob_of[id] * 4u;
                const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2];
                const float *sv = g.snap_tris + (size_t)id * 9u;
                const V3 v0 = V3{ sv[0], sv[1], sv[2] }, v1 = V3{ sv[3], sv[4], sv[5] }, v2 = V3{ sv[6], sv[7], sv[8] };
                const V3 e1 = v1 - v0, e2 = v2 - v0;
                moved = differs(v0, xyz(r0)) || differs(e1, xyz(r1)) || differs(e2, xyz(r2));
                if (moved) {
                    float u, v;
                    tri_uv(r0, r1, r2, o, d, u, v);
                    P = V3{ fma_(v, e2.x, fma_(u, e1.x, v0.x)), fma_(v, e2.y, fma_(u, e1.y, v0.y)), fma_(v, e2.z, fma_(u, e1.z, v0.z)) };
                    const V3 ng = normalize(cross(e1, e2));
                    wv = P - o2;
                    n = dot(ng, wv) < 0.0f ? ng : neg(ng);
                }
            } else if (id - g.n_tris < g.n_spheres) {
                const float4 sp = g.spheres[id - g.n_tris], ss = g.snap_spheres[id - g.n_tris];
                moved = differs(xyz(ss), xyz(sp)) || differs(ss.w, sp.w);
                if (moved) {
                    const float k = ss.w / sp.w;
                    P = V3{ fma_(P.x - sp.x, k, ss.x), fma_(P.y - sp.y, k, ss.y), fma_(P.z - sp.z, k, ss.z) };
                    wv = P - o2;
                }
            }
            s = gather_history(a, x, y, a.same_camera && !moved, P, n, wv, id);
        }
        float l;
        const float4 out = blend(a, c, s, l);
        took = store_pixel(a, ip, out, l);
    }
    // k_temporal's counter scheme, once for each of the two counts
    const unsigned long long m = __ballot(took), mm = __ballot(moved);
    if (threadIdx.x == 0u && (m | mm)) {
        const uint32_t line = counter_line();
        if (m) atomicAdd(a.taken + line, (uint32_t)__popcll(m));
        if (mm) atomicAdd(g.moved + line, (uint32_t)__popcll(mm));
    }
}

static void kernel_args(const TemporalArgs &t, TemporalKernelArgs &a)
{
    static_assert(sizeof(Camera) == sizeof(pt_camera), "camera layout");
    std::memcpy(&a.cam, &t.cam, sizeof a.cam);
    std::memcpy(&a.old_cam, &t.old_cam, sizeof a.old_cam);
    a.cam.jitter = 0u; a.old_cam.jitter = 0u;
    a.width = t.width; a.height = t.height;
    a.has_history = t.has_history; a.same_camera = t.same_camera; a.match_ids = t.match_ids;
    a.max_history = t.max_history; a.tau_p2 = t.tau_p2; a.tau_n = t.tau_n;
    a.frame = t.frame; a.g0 = t.g0; a.g1 = t.g1; a.old_g0 = t.old_g0; a.old_g1 = t.old_g1; a.old_h = t.old_h;
    a.out = t.out; a.new_h = t.new_h; a.taken = t.taken;
}

hipError_t launch_temporal(hipStream_t s, const TemporalArgs &t)
{
    TemporalKernelArgs a;
    kernel_args(t, a);
    hipLaunchKernelGGL(k_temporal, dim3((t.width + 63u) / 64u, (t.height + 3u) / 4u, 1u), dim3(64, 4, 1), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_temporal_motion(hipStream_t s, const TemporalArgs &t, const MotionArgs &m)
{
    if (!t.has_history) return hipErrorInvalidValue; // the kernel reads the history unconditionally
    TemporalKernelArgs a;
    kernel_args(t, a);
    const MotionKernelArgs g{ m.blob_of, m.tris, m.spheres, m.snap_tris, m.snap_spheres, m.n_tris, m.n_spheres, m.moved };
    hipLaunchKernelGGL(k_temporal_motion, dim3((t.width + 63u) / 64u, (t.height + 3u) / 4u, 1u), dim3(64, 4, 1), 0, s, a, g);
    return hipGetLastError();
}

} // namespace ptrt
