// query.cpp — ray queries (pt_trace_rays, docs/SPEC.md §4.2) and the host side of pt_denoise (docs/SPEC.md §8) with its read-backs, both
// over the query plumbing of context.h (Queries).
#include "scene.h"
#include "denoise.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

using namespace ptrt;

namespace {
constexpr uint64_t kTraceChunk = 1ull << 31;                   // rays per launch (k_trace indexes with 32 bits)
constexpr uint32_t kTraceWords = kCntTotalWords - kCntGlobals; // the counter words of a query: error flag first, then the visit counters
}

pt_status Queries::setup(pt_context *c, uint32_t overflow, uint64_t n_rays, PathState &ps)
{
    const uint32_t blocks = trace_blocks((uint32_t)std::min<uint64_t>(n_rays, kTraceChunk)), lanes = blocks * kExtBlock;
    ps = PathState{};
    ps.shard_cap = (lanes + kShards - 1u) / kShards; // one overflow column per lane of the grid, reused by its every ray
    ps.stack_ovf_entries = overflow;
    if (ps.stack_ovf_entries) HIP_TRY(c, ovf.ensure((size_t)ps.stack_ovf_entries * kShards * ps.shard_cap));
    ps.stack_ovf = ovf.p;
    HIP_TRY(c, cnt.ensure(kCntTotalWords)); // the kernels use the global words only: error flag and visit counters
    ps.counters = cnt.p;
    HIP_TRY(c, hipMemsetAsync(cnt.p + kCntGlobals, 0, sizeof(uint32_t) * kTraceWords, context_stream(c)));
    return PT_OK;
}
pt_status Queries::launch(pt_context *c, const DeviceScene &ds, const PathState &ps, const float4 *rays, float4 *hits, uint64_t n_rays,
                          bool occlusion, bool count)
{
    for (uint64_t first = 0; first < n_rays; first += kTraceChunk)
        HIP_TRY(c, launch_trace(context_stream(c), ds, ps, rays + 2u * first, hits + first, (uint32_t)std::min(kTraceChunk, n_rays - first), occlusion, count));
    return PT_OK;
}
pt_status Queries::finish(pt_context *c, Counts &out)
{
    uint32_t words[kTraceWords];
    HIP_TRY(c, hipMemcpyAsync(words, cnt.p + kCntGlobals, sizeof words, hipMemcpyDeviceToHost, context_stream(c)));
    HIP_TRY(c, hipStreamSynchronize(context_stream(c)));
    const CounterView hc{ words, kCntGlobals };
    out = Counts{ hc.error(), hc.u64(kCntNodes), hc.u64(kCntTris), hc.u64(kCntSph) };
    return PT_OK;
}

static pt_status trace_rays(pt_context *c, const pt_scene *s, const void *rays, void *hits, uint64_t n_rays, uint32_t flags, pt_stats *stats)
{
    constexpr uint32_t known = PT_TRACE_OCCLUSION | PT_TRACE_COUNT_VISITS | PT_TRACE_HOST_MEMORY;
    if (flags & ~known) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_trace_rays: unknown flag bits 0x%x", flags & ~known);
    const bool occlusion = (flags & PT_TRACE_OCCLUSION) != 0, count = (flags & PT_TRACE_COUNT_VISITS) != 0, host = (flags & PT_TRACE_HOST_MEMORY) != 0;
    if (occlusion && count) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_trace_rays: PT_TRACE_COUNT_VISITS counts closest-hit queries only (occlusion promises no visit order)");
    if (!c || !s || !rays || !hits) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_trace_rays: NULL argument");
    const uintptr_t align = host ? 3u : 15u; // the kernel loads and stores 16-byte rows; staged host arrays only need float alignment
    if (((uintptr_t)rays & align) || ((uintptr_t)hits & align))
        return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_trace_rays: rays and hits must be %u-byte aligned", (unsigned)align + 1u);
    if (s->ctx != c) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_trace_rays: scene belongs to another context");
    if (!s->committed) return fail(c, PT_ERR_NOT_COMMITTED, "scene not committed");
    if (n_rays >> 40) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_trace_rays: n_rays %llu is not a batch size", (unsigned long long)n_rays);
    pt_stats out{};
    out.rays = n_rays;
    if (n_rays == 0) { if (stats) *stats = out; return PT_OK; }
    HIP_TRY(c, hipSetDevice(c->device));
    pt_status st;
    if (!host && ((st = check_device_array(c, rays, n_rays * 32u, "rays")) != PT_OK || (st = check_device_array(c, hits, n_rays * 16u, "hits")) != PT_OK)) return st;
    hipStream_t q = c->stream;
    PathState ps;
    if ((st = c->query.setup(c, s->tree.stack_overflow(), n_rays, ps)) != PT_OK) return st;
    const float4 *d_rays = (const float4 *)rays;
    float4 *d_hits = (float4 *)hits;
    if (host) { // staged through the context's own buffers
        HIP_TRY(c, c->query.rays.ensure((size_t)n_rays * 2u)); HIP_TRY(c, c->query.hits.ensure((size_t)n_rays));
        HIP_TRY(c, hipMemcpyAsync(c->query.rays.p, rays, n_rays * 32u, hipMemcpyHostToDevice, q));
        d_rays = c->query.rays.p; d_hits = c->query.hits.p;
    }
    HIP_TRY(c, hipEventRecord(c->query.ev[0], q));
    if ((st = c->query.launch(c, s->ds, ps, d_rays, d_hits, n_rays, occlusion, count)) != PT_OK) return st;
    HIP_TRY(c, hipEventRecord(c->query.ev[1], q));
    if (host) HIP_TRY(c, hipMemcpyAsync(hits, d_hits, n_rays * 16u, hipMemcpyDeviceToHost, q));
    Queries::Counts n;
    if ((st = c->query.finish(c, n)) != PT_OK) return st;
    if (n.error) return fail(c, PT_ERR_INTERNAL, "pt_trace_rays: device error flag 0x%x (1 = traversal stack overflow, 2 = step limit)", n.error);
    float ms = 0.f; HIP_TRY(c, hipEventElapsedTime(&ms, c->query.ev[0], c->query.ev[1])); out.gpu_ms = ms;
    if (count) { out.node_visits = n.node_visits; out.tri_tests = n.tri_tests; out.sphere_tests = n.sphere_tests; }
    if (stats) *stats = out;
    return PT_OK;
}

extern "C" pt_status pt_trace_rays(pt_context *c, const pt_scene *s, const void *rays, void *hits, uint64_t n_rays, uint32_t flags, pt_stats *stats)
{
    return drained_on_failure(c, [&] { return trace_rays(c, s, rays, hits, n_rays, flags, stats); }); // (e.g. a copy into `hits`)
}


// ------------------------------------------------------------------------------------------------ denoising (docs/SPEC.md §8)

// §8.2 defaults, the exact f32 values SPEC §8.2 states (chosen by the quality sweep of tools/exp_denoise.py)
constexpr uint32_t kDenoiseIterations = 4u;
constexpr float kSigmaColor = 16.0f, kSigmaNormal = 0.0625f, kSigmaDepth = 0.0078125f, kSigmaAlbedo = 0.25f;

static pt_status denoise(pt_context *c, const pt_scene *s, const pt_denoise_params *dp, pt_stats *stats)
{
    if (!dp) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_denoise: dp is NULL");
    constexpr uint32_t known = PT_DENOISE_GUIDES_ONLY | PT_DENOISE_NO_EDGE_STOPS;
    if (dp->flags & ~known) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_denoise: unknown flag bits 0x%x", dp->flags & ~known);
    if (dp->iterations > 8u) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_denoise: iterations %u (0 = default, at most 8)", dp->iterations);
    const float sigma[4] = { dp->sigma_color, dp->sigma_normal, dp->sigma_depth, dp->sigma_albedo };
    static const char *const sigma_name[4] = { "sigma_color", "sigma_normal", "sigma_depth", "sigma_albedo" };
    for (int k = 0; k < 4; ++k)
        if (!(sigma[k] >= 0.0f) || std::isinf(sigma[k]))
            return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_denoise: %s = %g (must be finite and >= 0; 0 = default)", sigma_name[k], (double)sigma[k]);
    if (!c || !s) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_denoise: NULL context or scene");
    if (s->ctx != c) return fail(c, PT_ERR_UNSUPPORTED, "pt_denoise: the scene is %s", s->ctx ? "of another context" : "detached (no device copy to trace)");
    if (!s->committed) return fail(c, PT_ERR_NOT_COMMITTED, "pt_denoise: scene not committed");
    FrameOutputs &o = c->out;
    if (o.holds() == FrameOutputs::Holds::reference_sphere) return fail(c, PT_ERR_UNSUPPORTED, "pt_denoise: the framebuffer holds a PT_REFERENCE_SPHERE frame");
    if (!o.readable()) return fail(c, PT_ERR_NOT_COMMITTED, "pt_denoise: no assembled frame (render with nranks == 1 or assemble the tiles first)");
    const bool guides_only = (dp->flags & PT_DENOISE_GUIDES_ONLY) != 0;
    const uint32_t passes = guides_only ? 0u : dp->iterations ? dp->iterations : kDenoiseIterations;
    const float sc = sigma[0] != 0.0f ? sigma[0] : kSigmaColor, sn = sigma[1] != 0.0f ? sigma[1] : kSigmaNormal;
    const float sz = sigma[2] != 0.0f ? sigma[2] : kSigmaDepth, sa = sigma[3] != 0.0f ? sigma[3] : kSigmaAlbedo;

    const uint32_t w = o.width(), h = o.height(); // of the frame it filters
    const size_t n = (size_t)w * h;
    HIP_TRY(c, hipSetDevice(c->device));
    for (auto &e : o.ev_denoise) HIP_TRY(c, e.create());
    o.drop_denoised(); // from here on the buffers are rewritten
    HIP_TRY(c, o.dn_work.ensure(2 * n)); HIP_TRY(c, o.dn_hits.ensure(n));
    HIP_TRY(c, o.dn_g0.ensure(n)); HIP_TRY(c, o.dn_g1.ensure(n));
    if (passes) HIP_TRY(c, o.dn_out.ensure(n));
    const uint32_t nt = s->ds.n_tris;
    if (!s->cache.blob_of_ready) HIP_TRY(c, s->cache.d_blob_of.ensure(std::max<size_t>(nt, 1)));
    pt_status st;
    PathState ps;
    if ((st = c->query.setup(c, s->tree.stack_overflow(), n, ps)) != PT_OK) return st;
    hipStream_t q = c->stream;
    HIP_TRY(c, hipEventRecord(o.ev_denoise[0], q));
    if (!s->cache.blob_of_ready) { // (zeroed first: every entry is a valid blob index even if an id were missing)
        HIP_TRY(c, hipMemsetAsync(s->cache.d_blob_of.p, 0, std::max<size_t>(nt, 1) * sizeof(uint32_t), q));
        HIP_TRY(c, launch_guide_index(q, s->ds.tris, nt, s->cache.d_blob_of.p));
    }
    float4 *rays = o.dn_work.p;
    HIP_TRY(c, launch_guide_rays(q, s->cam, w, h, rays));
    if ((st = c->query.launch(c, s->ds, ps, rays, o.dn_hits.p, n, false, false)) != PT_OK) return st;
    HIP_TRY(c, launch_guide_resolve(q, s->ds, s->cache.d_blob_of.p, rays, o.dn_hits.p, (uint32_t)n, o.dn_g0.p, o.dn_g1.p));
    HIP_TRY(c, hipEventRecord(o.ev_denoise[1], q));
    // pass i reads the framebuffer (i = 0) or pass i-1's image; the last pass writes dn_out, the others alternate between the two halves
    // of dn_work (the rays are dead by then)
    AtrousParams ap{};
    ap.width = w; ap.height = h; ap.edge_stops = (dp->flags & PT_DENOISE_NO_EDGE_STOPS) == 0;
    ap.inv_sn = atrous_scale(1.0f / sn); ap.sigma_z = sz; ap.ia = atrous_scale(1.0f / (sa * sa));
    const float ic = 1.0f / (sc * sc);
    const float4 *src = o.fb.p;
    for (uint32_t i = 0; i < passes; ++i) {
        float4 *dst = i + 1 == passes ? o.dn_out.p : o.dn_work.p + (i & 1u) * n;
        ap.pass = i; ap.ic_i = atrous_scale(ic * (float)(1u << (2u * i)));
        HIP_TRY(c, launch_atrous(q, ap, src, o.dn_g0.p, o.dn_g1.p, dst));
        src = dst;
    }
    HIP_TRY(c, hipEventRecord(o.ev_denoise[2], q)); // (before the counters' read-back: one synchronise for both)
    Queries::Counts cn;
    if ((st = c->query.finish(c, cn)) != PT_OK) return st;
    if (cn.error) return fail(c, PT_ERR_INTERNAL, "pt_denoise: device error flag 0x%x in the guide pass (1 = traversal stack overflow, 2 = step limit)", cn.error);
    s->cache.blob_of_ready = true;
    float ms_guides = 0.f, ms_filter = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms_guides, o.ev_denoise[0], o.ev_denoise[1]));
    HIP_TRY(c, hipEventElapsedTime(&ms_filter, o.ev_denoise[1], o.ev_denoise[2]));
    pt_stats out{};
    out.rays = n; out.iterations = passes;
    out.extend_ms = ms_guides; out.other_ms = ms_filter; out.gpu_ms = (double)ms_guides + ms_filter;
    o.denoised(passes > 0);
    if (stats) *stats = out;
    return PT_OK;
}

extern "C" {

pt_status pt_denoise(pt_context *c, const pt_scene *s, const pt_denoise_params *dp, pt_stats *stats)
{
    return drained_on_failure(c, [&] { return denoise(c, s, dp, stats); });
}

pt_status pt_denoised_read(pt_context *c, float *rgba, uint64_t n_floats)
{
    if (!c || !rgba) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_denoised_read: NULL argument");
    if (!c->out.has_image()) return fail(c, PT_ERR_NOT_COMMITTED, "pt_denoised_read: no denoised image (pt_denoise after the last pt_render, without PT_DENOISE_GUIDES_ONLY)");
    return copy_out(c, rgba, c->out.dn_out.p, c->out.pixels() * 4, sizeof(float), n_floats, "floats");
}

pt_status pt_denoised_device_ptr(pt_context *c, void **dptr, uint64_t *n_floats)
{
    if (!c || !dptr) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_denoised_device_ptr: NULL argument");
    if (!c->out.has_image()) return fail(c, PT_ERR_NOT_COMMITTED, "pt_denoised_device_ptr: no denoised image");
    *dptr = c->out.dn_out.p;
    if (n_floats) *n_floats = c->out.pixels() * 4;
    return PT_OK;
}

pt_status pt_guides_read(pt_context *c, float *g8, uint64_t n_floats)
{
    if (!c || !g8) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_guides_read: NULL argument");
    if (!c->out.has_guides()) return fail(c, PT_ERR_NOT_COMMITTED, "pt_guides_read: no guides (pt_denoise after the last pt_render)");
    const size_t n = (size_t)c->out.pixels();
    if (n_floats < (uint64_t)n * 8) return fail(c, PT_ERR_INVALID_ARGUMENT, "buffer too small: need %llu floats", (unsigned long long)n * 8);
    HIP_TRY(c, hipSetDevice(c->device));
    std::vector<float4> planes(2 * n); // the device keeps g0 and g1 as separate planes (one coalesced row each for the filter)
    HIP_TRY(c, hipMemcpyAsync(planes.data(), c->out.dn_g0.p, n * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(planes.data() + n, c->out.dn_g1.p, n * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < n; ++i) {
        std::memcpy(g8 + 8 * i, &planes[i], sizeof(float4));
        std::memcpy(g8 + 8 * i + 4, &planes[n + i], sizeof(float4));
    }
    return PT_OK;
}

} // extern "C"
