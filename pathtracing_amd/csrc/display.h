// display.h — pt_display on the device (display.hip), docs/SPEC.md §10: a luminance histogram of the source, one wavefront that turns it
// into an exposure, and the tone pass that writes the 8-bit image. display_host.cpp owns the buffers (context.h FrameOutputs, DisplayAdaptation)
// and enqueues the three on the context's stream; nothing comes back to the host between them.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include "../../include/ptrt.h"

namespace ptrt {

// §10 defaults and limits, the exact f32 values SPEC §10 states
constexpr float kDisplayWhite = 4.0f, kDisplayKey = 0.18f;
constexpr float kDisplayExposureMin = 0x1p-40f, kDisplayExposureMax = 0x1p+40f, kDisplayLevelMin = 0x1p-20f, kDisplayLevelMax = 0x1p+20f;

constexpr uint32_t kDisplayBins = 512u;      // §10's bins: 8 per octave over [2^-32, 2^32)
constexpr uint32_t kDisplayInfoWords = 8u;   // a pt_display_info, as the device writes it
constexpr uint32_t kDisplayMeterWords = kDisplayBins + kDisplayInfoWords; // the meter block: the histogram, then the info record

// c_k of §10 for the n pixels of src, added into hist[0 .. 512) (zeroed by the caller)
hipError_t launch_display_histogram(hipStream_t s, const float4 *src, uint32_t n, uint32_t *hist);

struct DisplayResolveArgs {
    const uint32_t *hist;         // the 512 counts (not read without metering)
    uint32_t *info;               // kDisplayInfoWords words: the pt_display_info of this call; word 0 is E, which the tone pass reads
    const float *prev;            // E_prev (read only when have_state)
    float *next;                  // where E_a goes (written only when metering)
    bool metering, have_state;    // PT_DISPLAY_AUTO_EXPOSURE; an earlier call's exposure is there to adapt from
    float exposure, key, adapt;   // resolved (non-zero)
    uint32_t trim_low, trim_high;
};
hipError_t launch_display_resolve(hipStream_t s, const DisplayResolveArgs &a);

struct DisplayToneArgs {
    const float4 *src;            // n pixels
    const float *exposure;        // E on the device (the info record's first word)
    uint32_t *out;                // n words: R | G<<8 | B<<16 | A<<24
    uint32_t n, curve;            // PT_TONE_*
    float iw2;                    // PT_TONE_REINHARD: 1.0f / (white * white)
    bool linear;                  // PT_DISPLAY_LINEAR
};
hipError_t launch_display_tone(hipStream_t s, const DisplayToneArgs &a);

} // namespace ptrt
