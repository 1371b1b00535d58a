// quantize_node.h — the device quantiser of docs/SPEC.md §4.1 (layouts 68, 72, 73), shared by the GPU builder (lbvh.hip k_finalize)
// and the refit (refit.hip). bvh_build.cpp quantize_nodes is the host twin: the same grid, the same rounding, the same check.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ptrt {

__device__ __forceinline__ float quant_scale_of(uint32_t e) { return __uint_as_float(e << 23); }

// One node of N = 4 (64 bytes) or N = 8 (128 bytes) children. Per axis a power-of-two grid from the children's union; every decoded box
// encloses its float box, checked with the traversal's own expression fma((float)q, scale, origin). Writes origin | exponents (words
// 0-3) and the quantised coordinates (from byte 16 + 4N: qlo_x, qlo_y, qlo_z, qhi_x, qhi_y, qhi_z, N bytes each, child c in byte c);
// N = 4 also zeroes the pad words 14-15. The refs (words 4 .. 3 + N) are the caller's. Box: any type with float lo[3], hi[3].
template <int N, class Box>
__device__ __forceinline__ void quantize_node(const Box *box, const bool *used, uint32_t *w)
{
    static_assert(N == 4 || N == 8, "BVH4Q / BVH8Q nodes");
    constexpr int kW = N / 4; // u32 words per coordinate group
    float org[3]; uint32_t ex[3];
    uint32_t qlo[3][kW], qhi[3][kW];
    for (int a = 0; a < 3; ++a) {
        float lo = __builtin_inff(), hi = -__builtin_inff();
        for (int c = 0; c < N; ++c) if (used[c]) { lo = fminf(lo, box[c].lo[a]); hi = fmaxf(hi, box[c].hi[a]); }
        if (!(lo <= hi)) lo = hi = 0.f;
        org[a] = lo;
        int e = 1;
        {
            const float ext = hi - lo;
            int ee; const float m = frexpf(ext / 255.0f, &ee);
            e = (ext > 0.f) ? ee + 127 - (m == 0.5f ? 1 : 0) : 1;
            e = min(max(e, 1), 254);
        }
        for (;;) {
            const float sc = quant_scale_of((uint32_t)e);
            bool ok = true;
            uint32_t pl[kW], ph[kW];
            for (int k = 0; k < kW; ++k) pl[k] = ph[k] = 0u;
            for (int c = 0; c < N && ok; ++c) {
                if (!used[c]) continue;
                int ql = (int)floorf((box[c].lo[a] - lo) / sc), qh = (int)ceilf((box[c].hi[a] - lo) / sc);
                ql = min(max(ql, 0), 255); qh = min(max(qh, 0), 255);
                while (ql > 0 && !(__builtin_fmaf((float)ql, sc, lo) <= box[c].lo[a])) --ql;
                while (qh < 255 && !(__builtin_fmaf((float)qh, sc, lo) >= box[c].hi[a])) ++qh;
                if (!(__builtin_fmaf((float)ql, sc, lo) <= box[c].lo[a]) || !(__builtin_fmaf((float)qh, sc, lo) >= box[c].hi[a])) { ok = false; break; }
                pl[c / 4] |= (uint32_t)ql << (8 * (c % 4)); ph[c / 4] |= (uint32_t)qh << (8 * (c % 4));
            }
            if (ok || e >= 254) { for (int k = 0; k < kW; ++k) { qlo[a][k] = pl[k]; qhi[a][k] = ph[k]; } break; }
            ++e;
        }
        ex[a] = (uint32_t)e;
    }
    w[0] = __float_as_uint(org[0]); w[1] = __float_as_uint(org[1]); w[2] = __float_as_uint(org[2]);
    w[3] = ex[0] | (ex[1] << 8) | (ex[2] << 16);
    constexpr int q0 = 4 + N; // first word of the quantised coordinates
    for (int a = 0; a < 3; ++a)
        for (int k = 0; k < kW; ++k) { w[q0 + kW * a + k] = qlo[a][k]; w[q0 + kW * (3 + a) + k] = qhi[a][k]; }
    if (N == 4) { w[14] = 0u; w[15] = 0u; }
}

} // namespace ptrt
