// query.cpp — ray queries (pt_trace_rays, docs/SPEC.md §4.2) and the host side of pt_denoise (docs/SPEC.md §8) and pt_denoise_temporal
// (docs/SPEC.md §9) with their read-backs, all over the query plumbing of context.h (Queries); then the host side of pt_display
// (docs/SPEC.md §10), which post-processes what those calls and pt_render left.
#include "scene.h"
#include "denoise.h"
#include "temporal.h"
#include "display.h"
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

// What a checked pt_denoise_params asks for: the passes to run and the resolved (non-zero) sigmas
struct FilterPlan { uint32_t passes; float sc, sn, sz, sa; bool edge_stops; };

// pt_denoise's checks of dp, in pt_denoise's order (`who` names the public call in the error text)
static pt_status check_filter_params(pt_context *c, const char *who, const pt_denoise_params *dp, FilterPlan &plan)
{
    constexpr uint32_t known = PT_DENOISE_GUIDES_ONLY | PT_DENOISE_NO_EDGE_STOPS;
    if (dp->flags & ~known) return fail(c, PT_ERR_INVALID_ARGUMENT, "%s: unknown flag bits 0x%x", who, dp->flags & ~known);
    if (dp->iterations > 8u) return fail(c, PT_ERR_INVALID_ARGUMENT, "%s: iterations %u (0 = default, at most 8)", who, dp->iterations);
    const float sigma[4] = { dp->sigma_color, dp->sigma_normal, dp->sigma_depth, dp->sigma_albedo };
    static const char *const sigma_name[4] = { "sigma_color", "sigma_normal", "sigma_depth", "sigma_albedo" };
    for (int k = 0; k < 4; ++k)
        if (!(sigma[k] >= 0.0f) || std::isinf(sigma[k]))
            return fail(c, PT_ERR_INVALID_ARGUMENT, "%s: %s = %g (must be finite and >= 0; 0 = default)", who, sigma_name[k], (double)sigma[k]);
    const bool guides_only = (dp->flags & PT_DENOISE_GUIDES_ONLY) != 0;
    plan.passes = guides_only ? 0u : dp->iterations ? dp->iterations : kDenoiseIterations;
    plan.sc = sigma[0] != 0.0f ? sigma[0] : kSigmaColor; plan.sn = sigma[1] != 0.0f ? sigma[1] : kSigmaNormal;
    plan.sz = sigma[2] != 0.0f ? sigma[2] : kSigmaDepth; plan.sa = sigma[3] != 0.0f ? sigma[3] : kSigmaAlbedo;
    plan.edge_stops = (dp->flags & PT_DENOISE_NO_EDGE_STOPS) == 0;
    return PT_OK;
}

// pt_denoise's checks of the context, the scene and the framebuffer, in pt_denoise's order
static pt_status check_frame_to_denoise(pt_context *c, const char *who, const pt_scene *s)
{
    if (!c || !s) return fail(c, PT_ERR_INVALID_ARGUMENT, "%s: NULL context or scene", who);
    if (s->ctx != c) return fail(c, PT_ERR_UNSUPPORTED, "%s: the scene is %s", who, s->ctx ? "of another context" : "detached (no device copy to trace)");
    if (!s->committed) return fail(c, PT_ERR_NOT_COMMITTED, "%s: scene not committed", who);
    const FrameOutputs &o = c->out;
    if (o.holds() == FrameOutputs::Holds::reference_sphere) return fail(c, PT_ERR_UNSUPPORTED, "%s: the framebuffer holds a PT_REFERENCE_SPHERE frame", who);
    if (!o.readable()) return fail(c, PT_ERR_NOT_COMMITTED, "%s: no assembled frame (render with nranks == 1 or assemble the tiles first)", who);
    return PT_OK;
}

// §8.1 for the frame the framebuffer holds, into the planes g0 / g1 (w*h rows each): sizes the work buffers (and dn_out when `passes`),
// records ev_denoise[0], enqueues the guide rays, their trace and the resolve, records ev_denoise[1]. The caller finishes with
// c->query.finish() and, if that found no error, guides_done().
static pt_status guide_pass(pt_context *c, const pt_scene *s, uint32_t passes, float4 *g0, float4 *g1)
{
    FrameOutputs &o = c->out;
    const uint32_t w = o.width(), h = o.height(); // of the frame it filters
    const size_t n = (size_t)w * h;
    HIP_TRY(c, o.dn_work.ensure(2 * n)); HIP_TRY(c, o.dn_hits.ensure(n));
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
    HIP_TRY(c, launch_guide_resolve(q, s->ds, s->cache.d_blob_of.p, rays, o.dn_hits.p, (uint32_t)n, g0, g1));
    HIP_TRY(c, hipEventRecord(o.ev_denoise[1], q));
    return PT_OK;
}

// §8.2: plan.passes passes over `first` with the guides g0 / g1, then ev_denoise[2]. Pass i reads `first` (i = 0) or pass i-1's image; the
// last pass writes dn_out, the others alternate between the two halves of dn_work (the rays are dead by then)
static pt_status filter_passes(pt_context *c, const FilterPlan &plan, const float4 *first, const float4 *g0, const float4 *g1)
{
    FrameOutputs &o = c->out;
    const size_t n = (size_t)o.pixels();
    hipStream_t q = c->stream;
    AtrousParams ap{};
    ap.width = o.width(); ap.height = o.height(); ap.edge_stops = plan.edge_stops;
    ap.inv_sn = atrous_scale(1.0f / plan.sn); ap.sigma_z = plan.sz; ap.ia = atrous_scale(1.0f / (plan.sa * plan.sa));
    const float ic = 1.0f / (plan.sc * plan.sc);
    const float4 *src = first;
    for (uint32_t i = 0; i < plan.passes; ++i) {
        float4 *dst = i + 1 == plan.passes ? o.dn_out.p : o.dn_work.p + (i & 1u) * n;
        ap.pass = i; ap.ic_i = atrous_scale(ic * (float)(1u << (2u * i)));
        HIP_TRY(c, launch_atrous(q, ap, src, g0, g1, dst));
        src = dst;
    }
    HIP_TRY(c, hipEventRecord(o.ev_denoise[2], q)); // (before the counters' read-back: one synchronise for both)
    return PT_OK;
}

// The counters of the guide pass, behind one synchronise for everything the call enqueued
static pt_status guides_finish(pt_context *c, const char *who, const pt_scene *s)
{
    pt_status st;
    Queries::Counts cn;
    if ((st = c->query.finish(c, cn)) != PT_OK) return st;
    if (cn.error) return fail(c, PT_ERR_INTERNAL, "%s: device error flag 0x%x in the guide pass (1 = traversal stack overflow, 2 = step limit)", who, cn.error);
    s->cache.blob_of_ready = true;
    return PT_OK;
}

static pt_status denoise(pt_context *c, const pt_scene *s, const pt_denoise_params *dp, pt_stats *stats)
{
    static const char who[] = "pt_denoise";
    if (!dp) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_denoise: dp is NULL");
    pt_status st;
    FilterPlan plan;
    if ((st = check_filter_params(c, who, dp, plan)) != PT_OK || (st = check_frame_to_denoise(c, who, s)) != PT_OK) return st;
    FrameOutputs &o = c->out;
    const size_t n = (size_t)o.pixels();
    HIP_TRY(c, hipSetDevice(c->device));
    for (auto &e : o.ev_denoise) HIP_TRY(c, e.create());
    o.drop_denoised(); // from here on the buffers are rewritten
    HIP_TRY(c, o.dn_g0.ensure(n)); HIP_TRY(c, o.dn_g1.ensure(n));
    if ((st = guide_pass(c, s, plan.passes, o.dn_g0.p, o.dn_g1.p)) != PT_OK) return st;
    if ((st = filter_passes(c, plan, o.fb.p, o.dn_g0.p, o.dn_g1.p)) != PT_OK) return st;
    if ((st = guides_finish(c, who, s)) != PT_OK) return st;
    float ms_guides = 0.f, ms_filter = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms_guides, o.ev_denoise[0], o.ev_denoise[1]));
    HIP_TRY(c, hipEventElapsedTime(&ms_filter, o.ev_denoise[1], o.ev_denoise[2]));
    pt_stats out{};
    out.rays = n; out.iterations = plan.passes;
    out.extend_ms = ms_guides; out.other_ms = ms_filter; out.gpu_ms = (double)ms_guides + ms_filter;
    o.denoised(plan.passes > 0);
    if (stats) *stats = out;
    return PT_OK;
}

// ------------------------------------------------------------------------------------------------ temporal accumulation (docs/SPEC.md §9)

static pt_status denoise_temporal(pt_context *c, const pt_scene *s, const pt_temporal_params *tp, const pt_denoise_params *dp, pt_stats *stats)
{
    static const char who[] = "pt_denoise_temporal";
    if (!tp) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_denoise_temporal: tp is NULL");
    constexpr uint32_t known = PT_TEMPORAL_RESET | PT_TEMPORAL_MATCH_IDS | PT_TEMPORAL_MOTION;
    if (tp->flags & ~known) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_denoise_temporal: unknown flag bits 0x%x", tp->flags & ~known);
    if (tp->max_history > kTemporalMaxHistoryLimit)
        return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_denoise_temporal: max_history %u (0 = default, at most %u)", tp->max_history, kTemporalMaxHistoryLimit);
    if (!(tp->plane_tolerance >= 0.0f) || std::isinf(tp->plane_tolerance))
        return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_denoise_temporal: plane_tolerance = %g (must be finite and >= 0; 0 = default)", (double)tp->plane_tolerance);
    if (!(tp->normal_min >= 0.0f && tp->normal_min <= 1.0f))
        return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_denoise_temporal: normal_min = %g (0 = default, otherwise in (0, 1])", (double)tp->normal_min);
    pt_status st;
    FilterPlan plan{};
    if (dp && (st = check_filter_params(c, who, dp, plan)) != PT_OK) return st;
    if ((st = check_frame_to_denoise(c, who, s)) != PT_OK) return st;
    const uint32_t max_history = tp->max_history ? tp->max_history : kTemporalMaxHistory;
    const float tau_p = tp->plane_tolerance != 0.0f ? tp->plane_tolerance : kTemporalPlaneTolerance;
    const float tau_n = tp->normal_min != 0.0f ? tp->normal_min : kTemporalNormalMin;

    FrameOutputs &o = c->out;
    TemporalHistory &hist = c->history;
    const uint32_t w = o.width(), h = o.height();
    const size_t n = (size_t)w * h;
    HIP_TRY(c, hipSetDevice(c->device));
    for (auto &e : o.ev_denoise) HIP_TRY(c, e.create());
    HIP_TRY(c, o.ev_temporal.create());
    o.drop_denoised(); o.drop_temporal(); // from here on the buffers are rewritten (the history is not: this call writes its back planes)
    HIP_TRY(c, hist.reserve(w, h, kTemporalCounterWords));
    HIP_TRY(c, o.tm_out.ensure(n));
    HIP_TRY(c, hipMemsetAsync(hist.taken.p, 0, sizeof(uint32_t) * kTemporalCounterWords, c->stream)); // (ahead of the timed passes)
    const bool motion = (tp->flags & PT_TEMPORAL_MOTION) != 0;
    const TemporalHistory::SceneState state{ s->serial, s->updates, s->ds.n_tris, s->ds.n_spheres };
    if (motion) { // §9.1: the geometry this call is traced on, into the back set (ahead of the timed passes too)
        HIP_TRY(c, hist.reserve_snapshot(state, kTemporalCounterWords));
        const TemporalHistory::SnapshotTarget snap = hist.snapshot_back();
        const float *verts = nullptr;
        if ((st = s->verts.device(c, verts)) != PT_OK) return st; // (the buffer the last update wrote, or one upload of the host vector)
        if (state.n_tris) HIP_TRY(c, hipMemcpyAsync(snap.tris, verts, (size_t)state.n_tris * 36u, hipMemcpyDeviceToDevice, c->stream));
        if (state.n_spheres) HIP_TRY(c, hipMemcpyAsync(snap.spheres, s->ds.spheres, (size_t)state.n_spheres * 16u, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(c, hipMemsetAsync(hist.moved.p, 0, sizeof(uint32_t) * kTemporalCounterWords, c->stream));
    }
    const TemporalHistory::Target next = hist.back();
    if ((st = guide_pass(c, s, plan.passes, next.g0, next.g1)) != PT_OK) return st;
    hipStream_t q = c->stream;
    const TemporalHistory::Planes prev = hist.front();
    TemporalArgs ta{};
    ta.cam = s->cam; ta.old_cam = hist.camera();
    ta.width = w; ta.height = h;
    ta.has_history = hist.matches(w, h) && !(tp->flags & PT_TEMPORAL_RESET) && max_history != 1u;
    ta.same_camera = std::memcmp(&s->cam, &hist.camera(), sizeof(pt_camera)) == 0;
    ta.match_ids = (tp->flags & PT_TEMPORAL_MATCH_IDS) != 0;
    ta.max_history = (float)max_history; ta.tau_p2 = tau_p * tau_p; ta.tau_n = tau_n;
    ta.frame = o.fb.p; ta.g0 = next.g0; ta.g1 = next.g1;
    ta.old_g0 = prev.g0; ta.old_g1 = prev.g1; ta.old_h = prev.h;
    ta.out = o.tm_out.p; ta.new_h = next.h; ta.taken = hist.taken.p;
    // §9.1: the call uses the snapshot when it has a history whose snapshot was recorded from this scene and no commit since. If no
    // update has run since either, every pixel is unmoved and the pass is §9's
    const bool use_snapshot = motion && ta.has_history && hist.snapshot_of(state) && !hist.snapshot_is_current(state);
    if (use_snapshot) {
        const TemporalHistory::Snapshot was = hist.snapshot();
        MotionArgs ma{};
        ma.blob_of = s->cache.d_blob_of.p; ma.tris = s->ds.tris; ma.spheres = s->ds.spheres;
        ma.snap_tris = was.tris; ma.snap_spheres = was.spheres;
        ma.n_tris = state.n_tris; ma.n_spheres = state.n_spheres; ma.moved = hist.moved.p;
        HIP_TRY(c, launch_temporal_motion(q, ta, ma));
    } else HIP_TRY(c, launch_temporal(q, ta));
    HIP_TRY(c, hipEventRecord(o.ev_temporal, q));
    if ((st = filter_passes(c, plan, o.tm_out.p, next.g0, next.g1)) != PT_OK) return st;
    uint32_t lines[kTemporalCounterWords], moved_lines[kTemporalCounterWords];
    HIP_TRY(c, hipMemcpyAsync(lines, hist.taken.p, sizeof lines, hipMemcpyDeviceToHost, q)); // read behind guides_finish's synchronise
    if (use_snapshot) HIP_TRY(c, hipMemcpyAsync(moved_lines, hist.moved.p, sizeof moved_lines, hipMemcpyDeviceToHost, q));
    if ((st = guides_finish(c, who, s)) != PT_OK) return st;
    uint64_t taken = 0, moved = 0;
    for (uint32_t k = 0; k < kTemporalCounters; ++k) taken += lines[k * (kTemporalCounterWords / kTemporalCounters)];
    if (use_snapshot) for (uint32_t k = 0; k < kTemporalCounters; ++k) moved += moved_lines[k * (kTemporalCounterWords / kTemporalCounters)];
    float ms_guides = 0.f, ms_temporal = 0.f, ms_filter = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms_guides, o.ev_denoise[0], o.ev_denoise[1]));
    HIP_TRY(c, hipEventElapsedTime(&ms_temporal, o.ev_denoise[1], o.ev_temporal));
    HIP_TRY(c, hipEventElapsedTime(&ms_filter, o.ev_temporal, o.ev_denoise[2]));
    pt_stats out{};
    out.rays = n; out.paths = taken; out.iterations = plan.passes; out.reserved[0] = moved;
    out.extend_ms = ms_guides; out.shade_ms = ms_temporal; out.other_ms = ms_filter; out.gpu_ms = (double)ms_guides + ms_temporal + ms_filter;
    hist.commit(s->cam, w, h, motion ? &state : nullptr); // the back planes (and snapshot) are the history from here on
    o.denoised(plan.passes > 0, next.g0, next.g1);
    o.accumulated();
    if (stats) *stats = out;
    return PT_OK;
}

extern "C" {

pt_status pt_denoise(pt_context *c, const pt_scene *s, const pt_denoise_params *dp, pt_stats *stats)
{
    return drained_on_failure(c, [&] { return denoise(c, s, dp, stats); });
}

pt_status pt_denoise_temporal(pt_context *c, const pt_scene *s, const pt_temporal_params *tp, const pt_denoise_params *dp, pt_stats *stats)
{
    return drained_on_failure(c, [&] { return denoise_temporal(c, s, tp, dp, stats); });
}

pt_status pt_temporal_read(pt_context *c, float *rgba, uint64_t n_floats)
{
    if (!c || !rgba) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_temporal_read: NULL argument");
    if (!c->out.has_temporal()) return fail(c, PT_ERR_NOT_COMMITTED, "pt_temporal_read: no accumulated image (pt_denoise_temporal after the last pt_render)");
    return copy_out(c, rgba, c->out.tm_out.p, c->out.pixels() * 4, sizeof(float), n_floats, "floats");
}

pt_status pt_temporal_device_ptr(pt_context *c, void **dptr, uint64_t *n_floats)
{
    if (!c || !dptr) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_temporal_device_ptr: NULL argument");
    if (!c->out.has_temporal()) return fail(c, PT_ERR_NOT_COMMITTED, "pt_temporal_device_ptr: no accumulated image");
    *dptr = c->out.tm_out.p;
    if (n_floats) *n_floats = c->out.pixels() * 4;
    return PT_OK;
}

pt_status pt_temporal_history_read(pt_context *c, float *len, uint64_t n_floats)
{
    if (!c || !len) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_temporal_history_read: NULL argument");
    if (!c->out.has_temporal()) return fail(c, PT_ERR_NOT_COMMITTED, "pt_temporal_history_read: no history lengths (pt_denoise_temporal after the last pt_render)");
    const size_t n = (size_t)c->out.pixels();
    if (n_floats < (uint64_t)n) return fail(c, PT_ERR_INVALID_ARGUMENT, "buffer too small: need %llu floats", (unsigned long long)n);
    HIP_TRY(c, hipSetDevice(c->device));
    std::vector<float4> plane(n); // the history keeps a pixel's length in the .w of its accumulated colour
    HIP_TRY(c, hipMemcpyAsync(plane.data(), c->history.front().h, n * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < n; ++i) len[i] = plane[i].w;
    return PT_OK;
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
    const float4 *g0, *g1;             // (pt_denoise's own, or the history's after a pt_denoise_temporal)
    c->out.guides_from(g0, g1);
    HIP_TRY(c, hipMemcpyAsync(planes.data(), g0, n * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(planes.data() + n, g1, n * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < n; ++i) {
        std::memcpy(g8 + 8 * i, &planes[i], sizeof(float4));
        std::memcpy(g8 + 8 * i + 4, &planes[n + i], sizeof(float4));
    }
    return PT_OK;
}

} // extern "C"

// ------------------------------------------------------------------------------------------------ display (docs/SPEC.md §10)

// 0 means the default; anything else must lie in [lo, hi] (a NaN does not)
static bool display_level_ok(float v, float lo, float hi) { return v == 0.0f || (v >= lo && v <= hi); }

static pt_status display(pt_context *c, const pt_display_params *dp, pt_stats *stats)
{
    if (!dp) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_display: dp is NULL");
    if (dp->source > (uint32_t)PT_DISPLAY_TEMPORAL) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_display: unknown source %u", dp->source);
    if (dp->curve > (uint32_t)PT_TONE_ACES) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_display: unknown curve %u", dp->curve);
    constexpr uint32_t known = PT_DISPLAY_AUTO_EXPOSURE | PT_DISPLAY_LINEAR | PT_DISPLAY_RESET_ADAPTATION;
    if (dp->flags & ~known) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_display: unknown flag bits 0x%x", dp->flags & ~known);
    if (!display_level_ok(dp->exposure, kDisplayExposureMin, kDisplayExposureMax))
        return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_display: exposure = %g (0 = 1, otherwise in [2^-40, 2^40])", (double)dp->exposure);
    if (!display_level_ok(dp->white, kDisplayLevelMin, kDisplayLevelMax))
        return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_display: white = %g (0 = default, otherwise in [2^-20, 2^20])", (double)dp->white);
    if (!display_level_ok(dp->key, kDisplayLevelMin, kDisplayLevelMax))
        return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_display: key = %g (0 = default, otherwise in [2^-20, 2^20])", (double)dp->key);
    if (!(dp->adapt >= 0.0f && dp->adapt <= 1.0f))
        return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_display: adapt = %g (0 = 1, otherwise in (0, 1])", (double)dp->adapt);
    if ((uint64_t)dp->trim_low + dp->trim_high >= 1000u)
        return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_display: trim_low + trim_high = %llu per mille (must be below 1000)", (unsigned long long)dp->trim_low + dp->trim_high);
    if (!c) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_display: NULL context");
    FrameOutputs &o = c->out;
    const float4 *src = nullptr;
    switch (dp->source) {
    case PT_DISPLAY_FRAME:
        if (!o.readable()) return fail(c, PT_ERR_NOT_COMMITTED, "pt_display: no assembled frame (render with nranks == 1 or assemble the tiles first)");
        src = o.fb.p; break;
    case PT_DISPLAY_DENOISED:
        if (!o.has_image()) return fail(c, PT_ERR_NOT_COMMITTED, "pt_display: no denoised image (pt_denoise after the last pt_render, without PT_DENOISE_GUIDES_ONLY)");
        src = o.dn_out.p; break;
    default:
        if (!o.has_temporal()) return fail(c, PT_ERR_NOT_COMMITTED, "pt_display: no accumulated image (pt_denoise_temporal after the last pt_render)");
        src = o.tm_out.p; break;
    }
    const bool metering = (dp->flags & PT_DISPLAY_AUTO_EXPOSURE) != 0, reset = (dp->flags & PT_DISPLAY_RESET_ADAPTATION) != 0;
    const float white = dp->white != 0.0f ? dp->white : kDisplayWhite;
    DisplayAdaptation &state = c->adaptation;
    const uint32_t n = (uint32_t)o.pixels(); // at most 2^30 (layout_of)
    HIP_TRY(c, hipSetDevice(c->device));
    for (auto &e : o.ev_display) HIP_TRY(c, e.create());
    HIP_TRY(c, state.reserve());
    o.drop_display(); // from here on the buffers are rewritten (the adaptation state is not: this call writes its back slot)
    HIP_TRY(c, o.disp8.ensure(n)); HIP_TRY(c, o.disp_meter.ensure(kDisplayMeterWords));
    hipStream_t q = c->stream;
    uint32_t *hist = o.disp_meter.p, *info = o.disp_meter.p + kDisplayBins;
    HIP_TRY(c, hipEventRecord(o.ev_display[0], q));
    HIP_TRY(c, hipMemsetAsync(hist, 0, sizeof(uint32_t) * kDisplayBins, q));
    if (metering) HIP_TRY(c, launch_display_histogram(q, src, n, hist));
    DisplayResolveArgs ra{};
    ra.hist = hist; ra.info = info; ra.prev = state.front(); ra.next = state.back();
    ra.metering = metering; ra.have_state = metering && state.valid() && !reset;
    ra.exposure = dp->exposure != 0.0f ? dp->exposure : 1.0f;
    ra.key = dp->key != 0.0f ? dp->key : kDisplayKey; ra.adapt = dp->adapt != 0.0f ? dp->adapt : 1.0f;
    ra.trim_low = dp->trim_low; ra.trim_high = dp->trim_high;
    HIP_TRY(c, launch_display_resolve(q, ra));
    HIP_TRY(c, hipEventRecord(o.ev_display[1], q));
    DisplayToneArgs ta{};
    ta.src = src; ta.exposure = (const float *)info; ta.out = o.disp8.p; ta.n = n; ta.curve = dp->curve;
    ta.iw2 = 1.0f / (white * white); ta.linear = (dp->flags & PT_DISPLAY_LINEAR) != 0;
    HIP_TRY(c, launch_display_tone(q, ta));
    HIP_TRY(c, hipEventRecord(o.ev_display[2], q));
    HIP_TRY(c, hipStreamSynchronize(q));
    float ms_meter = 0.f, ms_tone = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms_meter, o.ev_display[0], o.ev_display[1]));
    HIP_TRY(c, hipEventElapsedTime(&ms_tone, o.ev_display[1], o.ev_display[2]));
    pt_stats out{};
    out.paths = n; out.extend_ms = ms_meter; out.other_ms = ms_tone; out.gpu_ms = (double)ms_meter + ms_tone;
    if (metering) state.commit(); // the back slot is the state from here on
    else if (reset) state.drop();
    o.displayed();
    if (stats) *stats = out;
    return PT_OK;
}

extern "C" {

pt_status pt_display(pt_context *c, const pt_display_params *dp, pt_stats *stats)
{
    return drained_on_failure(c, [&] { return display(c, dp, stats); });
}

pt_status pt_display_read(pt_context *c, uint8_t *rgba8, uint64_t n_bytes)
{
    if (!c || !rgba8) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_display_read: NULL argument");
    if (!c->out.has_display()) return fail(c, PT_ERR_NOT_COMMITTED, "pt_display_read: no displayed image (pt_display after the last pt_render)");
    return copy_out(c, rgba8, c->out.disp8.p, c->out.pixels() * 4, 1, n_bytes, "bytes");
}

pt_status pt_display_device_ptr(pt_context *c, void **dptr, uint64_t *n_bytes)
{
    if (!c || !dptr) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_display_device_ptr: NULL argument");
    if (!c->out.has_display()) return fail(c, PT_ERR_NOT_COMMITTED, "pt_display_device_ptr: no displayed image");
    *dptr = c->out.disp8.p;
    if (n_bytes) *n_bytes = c->out.pixels() * 4;
    return PT_OK;
}

pt_status pt_display_info_read(pt_context *c, pt_display_info *out)
{
    static_assert(sizeof(pt_display_info) == sizeof(uint32_t) * kDisplayInfoWords && sizeof(pt_display_params) == 40, "display struct layout");
    if (!c || !out) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_display_info_read: NULL argument");
    if (!c->out.has_display()) return fail(c, PT_ERR_NOT_COMMITTED, "pt_display_info_read: no displayed image (pt_display after the last pt_render)");
    return copy_out(c, out, c->out.disp_meter.p + kDisplayBins, kDisplayInfoWords, sizeof(uint32_t), kDisplayInfoWords, "words");
}

pt_status pt_display_histogram_read(pt_context *c, uint32_t *bins, uint64_t n_words)
{
    if (!c || !bins) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_display_histogram_read: NULL argument");
    if (!c->out.has_display()) return fail(c, PT_ERR_NOT_COMMITTED, "pt_display_histogram_read: no displayed image (pt_display after the last pt_render)");
    return copy_out(c, bins, c->out.disp_meter.p, kDisplayBins, sizeof(uint32_t), n_words, "words");
}

} // extern "C"
