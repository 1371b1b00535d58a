// temporal.hip — pt_denoise_temporal (docs/SPEC.md §9) on gfx950: reprojection of the previous call's history and the blend with the
// assembled frame, one fused kernel per call.
//
//   k_temporal : 64x4 workgroups as k_atrous: a wave covers 64 pixels of one row, so the centre reads (frame, g0, g1) and the two stores
//                are one coalesced 1 KiB row each. A pixel rebuilds its world position from its own guide depth, projects it through the
//                history's camera and takes up to four bilinear taps of the old guides and the old accumulated colour (length in .w);
//                under smooth motion neighbouring lanes land on neighbouring old pixels. Pixels that took history are counted by
//                ballot, one atomic per wave, spread over kTemporalCounters counter lines that the host adds up.
// Op order follows §9 exactly (explicit fma, -ffp-contract=off, IEEE division): tests/temporal_ref/ restates it bit for bit. Includes
// pt_device.h for the vector helpers and §3's camera ray only.
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
} // namespace

__global__ void __launch_bounds__(kBlock) k_temporal(TemporalKernelArgs a)
{
    const uint32_t x = blockIdx.x * 64u + threadIdx.x, y = blockIdx.y * 4u + threadIdx.y;
    bool took = false;
    if (x < a.width && y < a.height) {
        const size_t ip = (size_t)y * a.width + x;
        const float4 c = a.frame[ip];
        float4 out = c;
        float l = 1.0f;
        if (a.has_history) { // uniform over the grid
            const float4 ap = a.g1[ip];
            const uint32_t id = __float_as_uint(ap.w);
            if (id != PT_MISS) {
                const float4 np = a.g0[ip];
                const V3 n = xyz(np);
                V3 o, d;
                camera_ray(a.cam, x, y, 0u, o, d); // cam.jitter == 0: §8.1's ray
                const V3 P = madd(np.w, d, o);
                const V3 wv = P - V3{ a.old_cam.origin[0], a.old_cam.origin[1], a.old_cam.origin[2] };
                const float e2 = dot(wv, wv);
                TapSums s{ 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
                if (a.same_camera) {
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
                if (s.sw >= 0.25f) {
                    const float r = 1.0f / s.sw;
                    const float hr = s.sr * r, hg = s.sg * r, hb = s.sb * r;
                    l = fmin_(s.sl * r + 1.0f, a.max_history);
                    const float w = 1.0f / l;
                    out = make_float4(fma_(w, c.x - hr, hr), fma_(w, c.y - hg, hg), fma_(w, c.z - hb, hb), c.w);
                }
            }
        }
        a.out[ip] = out;
        a.new_h[ip] = make_float4(out.x, out.y, out.z, l);
        took = l > 1.0f;
    }
    // a wave is one row segment (threadIdx.y); no lane has left, so lane 0 speaks for it. Consecutive waves add to consecutive counter
    // lines: tens of thousands of atomics on one address would take longer than the rest of the kernel (ptrt_internal.h kShards)
    const unsigned long long m = __ballot(took);
    if (threadIdx.x == 0u && m) {
        const uint32_t wave = (blockIdx.y * gridDim.x + blockIdx.x) * 4u + threadIdx.y;
        atomicAdd(a.taken + (wave % kTemporalCounters) * kCounterStride, (uint32_t)__popcll(m));
    }
}

hipError_t launch_temporal(hipStream_t s, const TemporalArgs &t)
{
    static_assert(sizeof(Camera) == sizeof(pt_camera), "camera layout");
    TemporalKernelArgs a;
    std::memcpy(&a.cam, &t.cam, sizeof a.cam);
    std::memcpy(&a.old_cam, &t.old_cam, sizeof a.old_cam);
    a.cam.jitter = 0u; a.old_cam.jitter = 0u;
    a.width = t.width; a.height = t.height;
    a.has_history = t.has_history; a.same_camera = t.same_camera; a.match_ids = t.match_ids;
    a.max_history = t.max_history; a.tau_p2 = t.tau_p2; a.tau_n = t.tau_n;
    a.frame = t.frame; a.g0 = t.g0; a.g1 = t.g1; a.old_g0 = t.old_g0; a.old_g1 = t.old_g1; a.old_h = t.old_h;
    a.out = t.out; a.new_h = t.new_h; a.taken = t.taken;
    hipLaunchKernelGGL(k_temporal, dim3((t.width + 63u) / 64u, (t.height + 3u) / 4u, 1u), dim3(64, 4, 1), 0, s, a);
    return hipGetLastError();
}

} // namespace ptrt
