// display.hip — pt_display (docs/SPEC.md §10) on gfx950: metering, exposure and the tone pass, three kernels per call.
//
//   k_display_histogram : 256-thread workgroups in a grid-stride loop, one float4 load per lane and step (a wave reads 1 KiB). Each
//                         workgroup counts into a 512-word histogram in LDS, one LDS atomic per counted lane, and at its end adds its
//                         non-zero bins to the call's 512 words with global atomics: at most 2048 adds to one address per call, however
//                         flat the frame. (Agreeing on a wave's bins by ballot first, one LDS atomic per distinct bin, measured the
//                         same within the spread on rendered and on flat frames — DESIGN.md §13 — and was not kept.)
//   k_display_resolve   : one wavefront. A lane holds 8 consecutive bins; prefix counts through LDS give every bin the pixels below and
//                         above it, so the trim is a closed form per bin; lane 0 evaluates §10's u64 / f32 formulas and writes the
//                         info record (E first) and the next adaptation state. Nothing goes through the host.
//   k_display_tone      : the same grid-stride shape. The 255 thresholds are in LDS (1 KiB, filled once per workgroup); a channel's
//                         code is an 8-step binary search over them, which is the count of thresholds it reaches since they increase.
// Op order follows §10 exactly (explicit fma, -ffp-contract=off, IEEE division): tests/display_ref/ restates it bit for bit. Includes
// pt_device.h for fma_/fmin_ and §1's unorm8 only.
#include "ptrt_internal.h"
#include "pt_device.h"
#include "display.h"
#include "display_table.h"
#include <algorithm>

using namespace ptd;

namespace ptrt {

namespace {
constexpr uint32_t kDisplayMaxBlocks = 2048u; // 256 CUs x 8 workgroups: enough loads in flight, few enough flushes of one bin

PT_DEV uint32_t display_grid_stride() { return gridDim.x * kBlock; }

// §10's bin of a luminance; false: the pixel is not counted (Y <= 0 or NaN)
PT_DEV bool display_bin(float4 c, uint32_t &k)
{
    const float Y = fma_(0.0722f, c.z, fma_(0.7152f, c.y, 0.2126f * c.x));
    if (!(Y > 0.0f)) return false;
    const int b = (int)(__float_as_uint(Y) >> 20) - 760;
    k = (uint32_t)(b < 0 ? 0 : b > 511 ? 511 : b);
    return true;
}
} // namespace

__global__ void __launch_bounds__(kBlock) k_display_histogram(const float4 *__restrict__ src, uint32_t n, uint32_t *__restrict__ hist)
{
    __shared__ uint32_t bins[kDisplayBins];
    const uint32_t t = threadIdx.x;
    bins[t] = 0u; bins[t + kBlock] = 0u;
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + t; i < n; i += display_grid_stride()) {
        uint32_t k;
        if (display_bin(src[i], k)) atomicAdd(&bins[k], 1u);
    }
    __syncthreads();
    for (uint32_t b = t; b < kDisplayBins; b += kBlock) {
        const uint32_t v = bins[b];
        if (v) atomicAdd(hist + b, v);
    }
}

__global__ void __launch_bounds__(64) k_display_resolve(DisplayResolveArgs a)
{
    const uint32_t lane = threadIdx.x;
    float *info_f = (float *)a.info;
    if (!a.metering) { // E = exposure; nothing was metered
        if (lane == 0u) {
            info_f[0] = a.exposure;
            for (uint32_t w = 1u; w < kDisplayInfoWords; ++w) a.info[w] = 0u;
        }
        return;
    }
    __shared__ uint64_t part[64], part_s[64], part_n[64];
    uint32_t c[8];
    uint64_t mine = 0u;
#pragma unroll
    for (uint32_t j = 0; j < 8u; ++j) { c[j] = a.hist[lane * 8u + j]; mine += c[j]; }
    part[lane] = mine;
    __syncthreads();
    uint64_t below = 0u, N = 0u; // pixels in the bins of lower lanes; all counted pixels
    for (uint32_t l = 0; l < 64u; ++l) { const uint64_t v = part[l]; N += v; if (l < lane) below += v; }
    const uint64_t L = (N * a.trim_low) / 1000u, H = (N * a.trim_high) / 1000u;
    // L + H < N, so what is taken off the two ends never meets: bin k loses the part of [0, L) and of [N - H, N) that falls on its pixels
    uint64_t s = 0u, np = 0u;
#pragma unroll
    for (uint32_t j = 0; j < 8u; ++j) {
        const uint64_t ck = c[j], above = N - below - ck;
        const uint64_t lo = L > below ? (L - below < ck ? L - below : ck) : 0u;
        const uint64_t hi = H > above ? (H - above < ck ? H - above : ck) : 0u;
        const uint64_t kept = ck - lo - hi;
        s += (uint64_t)(lane * 8u + j) * kept; np += kept;
        below += ck;
    }
    part_s[lane] = s; part_n[lane] = np;
    __syncthreads();
    if (lane != 0u) return;
    uint64_t S = 0u, Np = 0u;
    for (uint32_t l = 0; l < 64u; ++l) { S += part_s[l]; Np += part_n[l]; }
    const float E_prev = a.have_state ? *a.prev : 0.0f;
    float E_t = 0.0f, Y_avg = 0.0f, E_a;
    if (N == 0u) E_a = a.have_state ? E_prev : 1.0f;
    else {
        const uint64_t A = 2u * S + Np, D = 16u * Np, q = A / D, r = A % D;
        // (r, D < 2^35 are exact as doubles, so each conversion rounds once, to nearest even)
        const float f = (float)(double)r / (float)(double)D;
        Y_avg = (1.0f + f) * __uint_as_float((uint32_t)(q + 95u) << 23); // 2^(q - 32)
        E_t = a.key / Y_avg;
        E_a = a.have_state ? fma_(a.adapt, E_t - E_prev, E_prev) : E_t;
    }
    *a.next = E_a;
    info_f[0] = E_a * a.exposure; info_f[1] = E_t; info_f[2] = Y_avg;
    a.info[3] = a.have_state ? 1u : 0u;
    a.info[4] = (uint32_t)N; a.info[5] = (uint32_t)(N >> 32);
    a.info[6] = (uint32_t)Np; a.info[7] = (uint32_t)(Np >> 32);
}

namespace {
// §10's pixel and curve for one channel: y in [0, 1]
template <uint32_t kCurve> PT_DEV float display_tone(float c, float E, float iw2)
{
    float x = c * E;
    x = (x > 0.0f) ? x : 0.0f;
    x = fmin_(x, 0x1p+20f);
    float y = x;
    if (kCurve == PT_TONE_REINHARD) y = (x * fma_(x, iw2, 1.0f)) / (1.0f + x);
    if (kCurve == PT_TONE_ACES) y = (x * fma_(2.51f, x, 0.03f)) / fma_(x, fma_(2.43f, x, 0.59f), 0.14f);
    return fmin_(y, 1.0f);
}
// the number of k in 1..255 with y >= T[k] (T increases)
PT_DEV uint32_t display_srgb8(const float *T, float y)
{
    uint32_t code = 0u;
#pragma unroll
    for (uint32_t step = 128u; step; step >>= 1) code += (y >= T[code + step]) ? step : 0u;
    return code;
}
} // namespace

template <uint32_t kCurve, bool kLinear> __global__ void __launch_bounds__(kBlock) k_display_tone(DisplayToneArgs a)
{
    __shared__ float T[256];
    if (!kLinear) { T[threadIdx.x] = kSrgb8Threshold[threadIdx.x]; __syncthreads(); }
    const float E = *a.exposure;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += display_grid_stride()) {
        const float4 c = a.src[i];
        const float r = display_tone<kCurve>(c.x, E, a.iw2), g = display_tone<kCurve>(c.y, E, a.iw2), b = display_tone<kCurve>(c.z, E, a.iw2);
        const uint32_t rgb = kLinear ? unorm8(r) | (unorm8(g) << 8) | (unorm8(b) << 16)
                                     : display_srgb8(T, r) | (display_srgb8(T, g) << 8) | (display_srgb8(T, b) << 16);
        a.out[i] = rgb | (unorm8(c.w) << 24);
    }
}

namespace {
uint32_t display_blocks(uint32_t n) { return std::min((n + kBlock - 1u) / kBlock, kDisplayMaxBlocks); }

template <uint32_t kCurve> void launch_tone_curve(hipStream_t s, const DisplayToneArgs &a)
{
    if (a.linear) hipLaunchKernelGGL((k_display_tone<kCurve, true>), dim3(display_blocks(a.n)), dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL((k_display_tone<kCurve, false>), dim3(display_blocks(a.n)), dim3(kBlock), 0, s, a);
}
} // namespace

hipError_t launch_display_histogram(hipStream_t s, const float4 *src, uint32_t n, uint32_t *hist)
{
    hipLaunchKernelGGL(k_display_histogram, dim3(display_blocks(n)), dim3(kBlock), 0, s, src, n, hist);
    return hipGetLastError();
}

hipError_t launch_display_resolve(hipStream_t s, const DisplayResolveArgs &a)
{
    hipLaunchKernelGGL(k_display_resolve, dim3(1), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_display_tone(hipStream_t s, const DisplayToneArgs &a)
{
    switch (a.curve) {
    case PT_TONE_CLAMP: launch_tone_curve<PT_TONE_CLAMP>(s, a); break;
    case PT_TONE_REINHARD: launch_tone_curve<PT_TONE_REINHARD>(s, a); break;
    case PT_TONE_ACES: launch_tone_curve<PT_TONE_ACES>(s, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

} // namespace ptrt
