// display_host.cpp — the host side of pt_display (docs/SPEC.md §10) with its read-backs and device pointer: post-processes what pt_render,
// pt_denoise or pt_denoise_temporal left. Owns what the call keeps: FrameOutputs' disp8 / disp_meter and DisplayAdaptation (context.h).
// The call is a list of phases: checks, pick the source, enqueue, finish and commit.
#include "context.h"
#include "display.h"
#include <hip/hip_runtime.h>

using namespace ptrt;

// 0 means the default; anything else must lie in [lo, hi] (a NaN does not)
static bool display_level_ok(float v, float lo, float hi) { return v == 0.0f || (v >= lo && v <= hi); }

// pt_display's checks of dp and then of the context, in its order
static pt_status check_display_params(pt_context *c, const pt_display_params *dp)
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
    return PT_OK;
}

// The image dp->source names, if the context has it
static pt_status display_source(pt_context *c, uint32_t source, const float4 *&src)
{
    const FrameOutputs &o = c->out;
    switch (source) {
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
    return PT_OK;
}

// §10 on the context's stream: ev_display[0], the histogram (zeroed; filled when metering), the resolve, ev_display[1], the tone pass over
// the n pixels of src, ev_display[2]. Nothing comes back to the host between them.
static pt_status enqueue_display(pt_context *c, const pt_display_params *dp, const float4 *src, uint32_t n)
{
    FrameOutputs &o = c->out;
    DisplayAdaptation &state = c->adaptation;
    const bool metering = (dp->flags & PT_DISPLAY_AUTO_EXPOSURE) != 0, reset = (dp->flags & PT_DISPLAY_RESET_ADAPTATION) != 0;
    const float white = dp->white != 0.0f ? dp->white : kDisplayWhite;
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
    return PT_OK;
}

static pt_status display(pt_context *c, const pt_display_params *dp, pt_stats *stats)
{
    pt_status st;
    const float4 *src = nullptr;
    if ((st = check_display_params(c, dp)) != PT_OK || (st = display_source(c, dp->source, src)) != PT_OK) return st;
    FrameOutputs &o = c->out;
    DisplayAdaptation &state = c->adaptation;
    const uint32_t n = (uint32_t)o.pixels(); // at most 2^30 (layout_of)
    HIP_TRY(c, hipSetDevice(c->device));
    for (auto &e : o.ev_display) HIP_TRY(c, e.create());
    HIP_TRY(c, state.reserve());
    o.drop_display(); // from here on the buffers are rewritten (the adaptation state is not: this call writes its back slot)
    HIP_TRY(c, o.disp8.ensure(n)); HIP_TRY(c, o.disp_meter.ensure(kDisplayMeterWords));
    if ((st = enqueue_display(c, dp, src, n)) != PT_OK) return st;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    float ms_meter = 0.f, ms_tone = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms_meter, o.ev_display[0], o.ev_display[1]));
    HIP_TRY(c, hipEventElapsedTime(&ms_tone, o.ev_display[1], o.ev_display[2]));
    pt_stats out{};
    out.paths = n; out.extend_ms = ms_meter; out.other_ms = ms_tone; out.gpu_ms = (double)ms_meter + ms_tone;
    if (dp->flags & PT_DISPLAY_AUTO_EXPOSURE) state.commit(); // the back slot is the state from here on
    else if (dp->flags & PT_DISPLAY_RESET_ADAPTATION) state.drop();
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
