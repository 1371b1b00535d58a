// query.cpp — ray queries (pt_trace_rays, docs/SPEC.md §4.2), hemisphere gathers (pt_gather, §12; pt_gather_paths, §12.1 and §12.2) and the query plumbing of context.h
// (Queries), which pt_denoise's guide pass shares (denoise_host.cpp).
#include "scene.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>

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

// pt_gather (docs/SPEC.md §12) and pt_gather_paths (§12.1): the rays are made, traced and reduced inside k_gather / k_gather_paths; the
// host only checks, stages and launches. paths: the call is pt_gather_paths (fn names it in messages) and pp its own parameters, checked
// before everything the two calls share.
static pt_status gather(pt_context *c, const pt_scene *s, const void *points, void *out_rows, uint64_t n_points, const pt_gather_params *gp, pt_stats *stats,
                        bool paths = false, const pt_gather_path_params *pp = nullptr)
{
    const char *fn = paths ? "pt_gather_paths" : "pt_gather";
    if (paths) {
        if (!pp) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_gather_paths: path params is NULL");
        const uint32_t known = PT_GATHER_PATHS_NEXT_EVENT | PT_GATHER_PATHS_SPHERE_LIGHTS;
        if (pp->flags & ~known) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_gather_paths: unknown path flag bits 0x%x", pp->flags & ~known);
        if ((pp->flags & PT_GATHER_PATHS_SPHERE_LIGHTS) && !(pp->flags & PT_GATHER_PATHS_NEXT_EVENT))
            return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_gather_paths: PT_GATHER_PATHS_SPHERE_LIGHTS needs PT_GATHER_PATHS_NEXT_EVENT");
        if (pp->max_depth > 255u) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_gather_paths: max_depth %u is more than 255", pp->max_depth);
    }
    if (!gp) return fail(c, PT_ERR_INVALID_ARGUMENT, "%s: params is NULL", fn);
    if (gp->flags & ~(uint32_t)PT_GATHER_HOST_MEMORY) return fail(c, PT_ERR_INVALID_ARGUMENT, "%s: unknown flag bits 0x%x", fn, gp->flags & ~(uint32_t)PT_GATHER_HOST_MEMORY);
    if (gp->samples > 4096u) return fail(c, PT_ERR_INVALID_ARGUMENT, "%s: samples %u is more than 4096", fn, gp->samples);
    if (!(gp->max_distance >= 0.0f) || std::isinf(gp->max_distance)) return fail(c, PT_ERR_INVALID_ARGUMENT, "%s: max_distance must be 0 (unbounded) or finite and positive", fn);
    if (!(gp->ray_eps >= 0.0f) || std::isinf(gp->ray_eps)) return fail(c, PT_ERR_INVALID_ARGUMENT, "%s: ray_eps must be finite and not negative", fn);
    const bool host = (gp->flags & PT_GATHER_HOST_MEMORY) != 0;
    if (!c || !s || !points || !out_rows) return fail(c, PT_ERR_INVALID_ARGUMENT, "%s: NULL argument", fn);
    const uintptr_t align = host ? 3u : 15u; // the kernel loads and stores 16-byte rows; staged host arrays only need float alignment
    if (((uintptr_t)points & align) || ((uintptr_t)out_rows & align))
        return fail(c, PT_ERR_INVALID_ARGUMENT, "%s: points and out must be %u-byte aligned", fn, (unsigned)align + 1u);
    if (s->ctx != c) return fail(c, PT_ERR_INVALID_ARGUMENT, "%s: scene belongs to another context", fn);
    if (!s->committed) return fail(c, PT_ERR_NOT_COMMITTED, "scene not committed");
    // docs/SPEC.md §13: a bake that ignored the textures would be wrong, and k_gather_paths has no textured form (pt_gather reads no albedo)
    if (paths && s->textures.textured()) return fail(c, PT_ERR_UNSUPPORTED, "pt_gather_paths: the scene is textured (pt_scene_set_material_textures); path gathers do not look textures up");
    if (n_points >> 32) return fail(c, PT_ERR_INVALID_ARGUMENT, "%s: n_points %llu is not a batch size", fn, (unsigned long long)n_points);
    pt_stats res{};
    res.paths = n_points;
    if (n_points == 0) { if (stats) *stats = res; return PT_OK; }
    GatherParams k{};
    k.samples = gp->samples ? gp->samples : 64u; k.seed = gp->seed;
    k.point_offset = gp->point_offset; k.sample_offset = gp->sample_offset;
    k.tmax = gp->max_distance > 0.0f ? gp->max_distance : INFINITY; k.ray_eps = gp->ray_eps;
    GatherPathParams kp{};
    if (paths) { kp.max_depth = pp->max_depth ? pp->max_depth : 8u; kp.rr_start = pp->rr_start; }
    HIP_TRY(c, hipSetDevice(c->device));
    pt_status st;
    if (!host && ((st = check_device_array(c, points, n_points * 32u, "points", fn, "PT_GATHER_HOST_MEMORY")) != PT_OK ||
                  (st = check_device_array(c, out_rows, n_points * 32u, "out", fn, "PT_GATHER_HOST_MEMORY")) != PT_OK)) return st;
    hipStream_t q = c->stream;
    PathState ps;
    // one overflow column per lane of the largest grid a launch of this call uses: setup sizes it for that many one-ray lanes
    const uint64_t lanes = (uint64_t)gather_blocks((uint32_t)std::min(n_points, kTraceChunk), k.samples) * kExtBlock;
    if ((st = c->query.setup(c, s->tree.stack_overflow(), lanes, ps)) != PT_OK) return st;
    const float4 *d_points = (const float4 *)points;
    float4 *d_out = (float4 *)out_rows;
    if (host) { // staged through the context's own buffers (two rows per point each way)
        HIP_TRY(c, c->query.rays.ensure((size_t)n_points * 2u)); HIP_TRY(c, c->query.hits.ensure((size_t)n_points * 2u));
        HIP_TRY(c, hipMemcpyAsync(c->query.rays.p, points, n_points * 32u, hipMemcpyHostToDevice, q));
        d_points = c->query.rays.p; d_out = c->query.hits.p;
    }
    // §12.2: a flagged call samples the scene's light set and its map if that is lit; with neither it is the unflagged call, kernel and all
    const bool env_lit = s->env.present() && s->env.lit();
    // §7.1: with PT_GATHER_PATHS_SPHERE_LIGHTS on a scene that has a sphere light "the table" is the joint table; without one the bit changes nothing
    const bool sph = paths && (pp->flags & PT_GATHER_PATHS_NEXT_EVENT) && (pp->flags & PT_GATHER_PATHS_SPHERE_LIGHTS) && s->n_sph_lights;
    const bool nee = paths && (pp->flags & PT_GATHER_PATHS_NEXT_EVENT) && (s->n_lights || env_lit || sph);
    const NeeArgs na = sph ? NeeArgs{ s->d_jlights.p, s->d_jcdf.p, s->d_jpa.p, s->n_lights + s->n_sph_lights, nullptr, nullptr }
                           : NeeArgs{ s->d_lights.p, s->d_cdf.p, s->d_pa.p, s->n_lights, nullptr, nullptr };
    const SphArgs sa{ s->d_sph_pmf.p, s->n_lights, 0u };
    const EnvArgs env = s->env.present() ? s->env.args(nee && env_lit && na.n_lights ? 0.5f : 1.0f) : EnvArgs{};
    HIP_TRY(c, hipEventRecord(c->query.ev[0], q));
    for (uint64_t first = 0; first < n_points; first += kTraceChunk) { // point_offset + first wraps like the key's own u32 arithmetic
        GatherParams kc = k; kc.point_offset = k.point_offset + (uint32_t)first;
        const uint32_t nc = (uint32_t)std::min(kTraceChunk, n_points - first);
        HIP_TRY(c, launch_gather(q, s->ds, ps, d_points + 2u * first, d_out + 2u * first, nc, kc, paths ? &kp : nullptr, s->env.present() ? &env : nullptr, nee ? &na : nullptr,
                                 sph ? &sa : nullptr));
    }
    HIP_TRY(c, hipEventRecord(c->query.ev[1], q));
    if (host) HIP_TRY(c, hipMemcpyAsync(out_rows, d_out, n_points * 32u, hipMemcpyDeviceToHost, q));
    Queries::Counts n;
    if ((st = c->query.finish(c, n)) != PT_OK) return st;
    if (n.error) return fail(c, PT_ERR_INTERNAL, "%s: device error flag 0x%x (1 = traversal stack overflow, 2 = step limit)", fn, n.error);
    float ms = 0.f; HIP_TRY(c, hipEventElapsedTime(&ms, c->query.ev[0], c->query.ev[1])); res.gpu_ms = ms;
    // the kernel counted the invalid points where the visit counter lives, and k_gather_paths its segments (and shadow rays) where the triangle tests' does
    res.rays = paths ? n.tri_tests : (uint64_t)k.samples * (n_points - n.node_visits);
    if (stats) *stats = res;
    return PT_OK;
}

extern "C" pt_status pt_gather_paths(pt_context *c, const pt_scene *s, const void *points, void *out, uint64_t n_points, const pt_gather_params *gp,
                                     const pt_gather_path_params *pp, pt_stats *stats)
{
    return drained_on_failure(c, [&] { return gather(c, s, points, out, n_points, gp, stats, true, pp); });
}

extern "C" pt_status pt_gather(pt_context *c, const pt_scene *s, const void *points, void *out, uint64_t n_points, const pt_gather_params *gp, pt_stats *stats)
{
    return drained_on_failure(c, [&] { return gather(c, s, points, out, n_points, gp, stats); }); // (e.g. a copy into `out`)
}

extern "C" pt_status pt_trace_rays(pt_context *c, const pt_scene *s, const void *rays, void *hits, uint64_t n_rays, uint32_t flags, pt_stats *stats)
{
    return drained_on_failure(c, [&] { return trace_rays(c, s, rays, hits, n_rays, flags, stats); }); // (e.g. a copy into `hits`)
}
