// denoise_host.cpp — the host side of pt_denoise (docs/SPEC.md §8) and pt_denoise_temporal (§9, §9.1) with their read-backs and device
// pointers, over the query plumbing of context.h (Queries, query.cpp). Owns what those calls keep: FrameOutputs' dn_* / tm_out buffers and
// TemporalHistory. Each call is a list of phases: checks, reserve, enqueue (guide pass, temporal pass, filter passes), finish, commit.
#include "scene.h"
#include "denoise.h"
#include "temporal.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

using namespace ptrt;

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
// guides_finish().
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
    const TexArgs tex = s->textures.args(); // docs/SPEC.md §13: on a textured scene g1.rgb = albedo * texel
    HIP_TRY(c, launch_guide_resolve(q, s->ds, s->cache.d_blob_of.p, rays, o.dn_hits.p, (uint32_t)n, g0, g1, s->textures.textured() ? &tex : nullptr));
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

// What a checked pt_temporal_params asks for: the flags and the three resolved (non-zero) levels
struct TemporalPlan { uint32_t max_history; float tau_p, tau_n; bool reset, match_ids, motion; };

// pt_denoise_temporal's checks of tp, in its order
static pt_status check_temporal_params(pt_context *c, const pt_temporal_params *tp, TemporalPlan &plan)
{
    if (!tp) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_denoise_temporal: tp is NULL");
    constexpr uint32_t known = PT_TEMPORAL_RESET | PT_TEMPORAL_MATCH_IDS | PT_TEMPORAL_MOTION;
    if (tp->flags & ~known) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_denoise_temporal: unknown flag bits 0x%x", tp->flags & ~known);
    if (tp->max_history > kTemporalMaxHistoryLimit)
        return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_denoise_temporal: max_history %u (0 = default, at most %u)", tp->max_history, kTemporalMaxHistoryLimit);
    if (!(tp->plane_tolerance >= 0.0f) || std::isinf(tp->plane_tolerance))
        return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_denoise_temporal: plane_tolerance = %g (must be finite and >= 0; 0 = default)", (double)tp->plane_tolerance);
    if (!(tp->normal_min >= 0.0f && tp->normal_min <= 1.0f))
        return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_denoise_temporal: normal_min = %g (0 = default, otherwise in (0, 1])", (double)tp->normal_min);
    plan.max_history = tp->max_history ? tp->max_history : kTemporalMaxHistory;
    plan.tau_p = tp->plane_tolerance != 0.0f ? tp->plane_tolerance : kTemporalPlaneTolerance;
    plan.tau_n = tp->normal_min != 0.0f ? tp->normal_min : kTemporalNormalMin;
    plan.reset = (tp->flags & PT_TEMPORAL_RESET) != 0; plan.match_ids = (tp->flags & PT_TEMPORAL_MATCH_IDS) != 0;
    plan.motion = (tp->flags & PT_TEMPORAL_MOTION) != 0;
    return PT_OK;
}

// §9.1: the geometry this call is traced on, into the history's back set, and the `moved` lines zeroed (ahead of the timed passes)
static pt_status record_snapshot(pt_context *c, const pt_scene *s, const TemporalHistory::SceneState &state)
{
    TemporalHistory &hist = c->history;
    HIP_TRY(c, hist.reserve_snapshot(state, kTemporalCounterWords));
    const TemporalHistory::SnapshotTarget snap = hist.snapshot_back();
    pt_status st;
    const float *verts = nullptr;
    if ((st = s->verts.device(c, verts)) != PT_OK) return st; // (the buffer the last update wrote, or one upload of the host vector)
    if (state.n_tris) HIP_TRY(c, hipMemcpyAsync(snap.tris, verts, (size_t)state.n_tris * 36u, hipMemcpyDeviceToDevice, c->stream));
    if (state.n_spheres) HIP_TRY(c, hipMemcpyAsync(snap.spheres, s->ds.spheres, (size_t)state.n_spheres * 16u, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(hist.moved.p, 0, sizeof(uint32_t) * kTemporalCounterWords, c->stream));
    return PT_OK;
}

// §9 / §9.1 after the guide pass wrote next.g0 / g1: the frame blended into the history's front set, into tm_out and next.h; then
// ev_temporal. `used_snapshot`: the pass was the motion kernel's, and hist.moved counts
static pt_status temporal_pass(pt_context *c, const pt_scene *s, const TemporalPlan &plan, const TemporalHistory::SceneState &state,
                               const TemporalHistory::Target &next, bool &used_snapshot)
{
    FrameOutputs &o = c->out;
    TemporalHistory &hist = c->history;
    hipStream_t q = c->stream;
    const TemporalHistory::Planes prev = hist.front();
    TemporalArgs ta{};
    ta.cam = s->cam; ta.old_cam = hist.camera();
    ta.width = o.width(); ta.height = o.height();
    ta.has_history = hist.matches(ta.width, ta.height) && !plan.reset && plan.max_history != 1u;
    ta.same_camera = std::memcmp(&s->cam, &hist.camera(), sizeof(pt_camera)) == 0;
    ta.match_ids = plan.match_ids;
    ta.max_history = (float)plan.max_history; ta.tau_p2 = plan.tau_p * plan.tau_p; ta.tau_n = plan.tau_n;
    ta.frame = o.fb.p; ta.g0 = next.g0; ta.g1 = next.g1;
    ta.old_g0 = prev.g0; ta.old_g1 = prev.g1; ta.old_h = prev.h;
    ta.out = o.tm_out.p; ta.new_h = next.h; ta.taken = hist.taken.p;
    // §9.1: the call uses the snapshot when it has a history whose snapshot was recorded from this scene and no commit since. If no
    // update has run since either, every pixel is unmoved and the pass is §9's
    used_snapshot = plan.motion && ta.has_history && hist.snapshot_of(state) && !hist.snapshot_is_current(state);
    if (used_snapshot) {
        const TemporalHistory::Snapshot was = hist.snapshot();
        MotionArgs ma{};
        ma.blob_of = s->cache.d_blob_of.p; ma.tris = s->ds.tris; ma.spheres = s->ds.spheres;
        ma.snap_tris = was.tris; ma.snap_spheres = was.spheres;
        ma.n_tris = state.n_tris; ma.n_spheres = state.n_spheres; ma.moved = hist.moved.p;
        HIP_TRY(c, launch_temporal_motion(q, ta, ma));
    } else HIP_TRY(c, launch_temporal(q, ta));
    HIP_TRY(c, hipEventRecord(o.ev_temporal, q));
    return PT_OK;
}

// The sum of a block of counter lines (`taken`, `moved`) read back from the device
static uint64_t sum_counter_lines(const uint32_t *lines)
{
    uint64_t sum = 0;
    for (uint32_t k = 0; k < kTemporalCounters; ++k) sum += lines[k * (kTemporalCounterWords / kTemporalCounters)];
    return sum;
}

static pt_status denoise_temporal(pt_context *c, const pt_scene *s, const pt_temporal_params *tp, const pt_denoise_params *dp, pt_stats *stats)
{
    static const char who[] = "pt_denoise_temporal";
    pt_status st;
    TemporalPlan tplan;
    FilterPlan plan{};
    if ((st = check_temporal_params(c, tp, tplan)) != PT_OK) return st;
    if (dp && (st = check_filter_params(c, who, dp, plan)) != PT_OK) return st;
    if ((st = check_frame_to_denoise(c, who, s)) != PT_OK) return st;

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
    hipStream_t q = c->stream;
    HIP_TRY(c, hipMemsetAsync(hist.taken.p, 0, sizeof(uint32_t) * kTemporalCounterWords, q)); // (ahead of the timed passes)
    const TemporalHistory::SceneState state{ s->serial, s->updates, s->ds.n_tris, s->ds.n_spheres };
    if (tplan.motion && (st = record_snapshot(c, s, state)) != PT_OK) return st;

    const TemporalHistory::Target next = hist.back();
    bool used_snapshot = false;
    if ((st = guide_pass(c, s, plan.passes, next.g0, next.g1)) != PT_OK) return st;
    if ((st = temporal_pass(c, s, tplan, state, next, used_snapshot)) != PT_OK) return st;
    if ((st = filter_passes(c, plan, o.tm_out.p, next.g0, next.g1)) != PT_OK) return st;
    uint32_t taken[kTemporalCounterWords], moved[kTemporalCounterWords];
    HIP_TRY(c, hipMemcpyAsync(taken, hist.taken.p, sizeof taken, hipMemcpyDeviceToHost, q)); // read behind guides_finish's synchronise
    if (used_snapshot) HIP_TRY(c, hipMemcpyAsync(moved, hist.moved.p, sizeof moved, hipMemcpyDeviceToHost, q));
    if ((st = guides_finish(c, who, s)) != PT_OK) return st;

    float ms_guides = 0.f, ms_temporal = 0.f, ms_filter = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms_guides, o.ev_denoise[0], o.ev_denoise[1]));
    HIP_TRY(c, hipEventElapsedTime(&ms_temporal, o.ev_denoise[1], o.ev_temporal));
    HIP_TRY(c, hipEventElapsedTime(&ms_filter, o.ev_temporal, o.ev_denoise[2]));
    pt_stats out{};
    out.rays = n; out.paths = sum_counter_lines(taken); out.iterations = plan.passes;
    out.reserved[0] = used_snapshot ? sum_counter_lines(moved) : 0u;
    out.extend_ms = ms_guides; out.shade_ms = ms_temporal; out.other_ms = ms_filter; out.gpu_ms = (double)ms_guides + ms_temporal + ms_filter;
    hist.commit(s->cam, w, h, tplan.motion ? &state : nullptr); // the back planes (and snapshot) are the history from here on
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
