// denoise.h — pt_denoise on the device (denoise.hip), docs/SPEC.md §8: the guide buffers of the first hit and the edge-aware à-trous
// filter. denoise_host.cpp owns the buffers and calls these in order: index (once per commit), guide rays, launch_trace (kernels.hip), resolve,
// then one à-trous launch per pass.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include "../../include/ptrt.h"

namespace ptrt {

struct DeviceScene;

// Original triangle id -> blob index, scattered from every blob record's row 0 .w (ids >= n_tris are dropped, never written).
hipError_t launch_guide_index(hipStream_t s, const float4 *tris, uint32_t n_tris, uint32_t *blob_of);
// §8.1 step 1: the unjittered §3 camera ray of every pixel of a w x h frame as a pt_trace_rays record {o | +inf, d | 0}.
hipError_t launch_guide_rays(hipStream_t s, const pt_camera &cam, uint32_t w, uint32_t h, float4 *rays);
// §8.1 step 3: the closest hits {t, prim id, u, v} of those rays -> g0 = (n, t), g1 = (albedo, prim id bits), one plane each.
hipError_t launch_guide_resolve(hipStream_t s, const DeviceScene &sc, const uint32_t *blob_of, const float4 *rays, const float4 *hits,
                                uint32_t n, float4 *g0, float4 *g1, const TexArgs *tex = nullptr); // tex: a textured scene's block (docs/SPEC.md §13: g1.rgb = albedo * texel), else NULL

// §8.2 pass `pass` (step 2^pass) of the filter: src -> dst, both w x h row-major float4. The sigmas are the resolved (non-zero) ones;
// every inverse scale is clamped into [2^-149, FLT_MAX] (atrous_scale).
struct AtrousParams {
    uint32_t width, height, pass;
    bool edge_stops;   // false: PT_DENOISE_NO_EDGE_STOPS
    float ic_i;        // clamp((1 / sigma_c^2) * 4^pass)
    float inv_sn;      // clamp(1 / sigma_n)
    float sigma_z;
    float ia;          // clamp(1 / sigma_a^2)
};
inline float atrous_scale(float v) { return v < 0x1p-149f ? 0x1p-149f : v > 3.40282347e+38f ? 3.40282347e+38f : v; }
hipError_t launch_atrous(hipStream_t s, const AtrousParams &p, const float4 *src, const float4 *g0, const float4 *g1, float4 *dst);

} // namespace ptrt
