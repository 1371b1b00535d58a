// temporal.h — pt_denoise_temporal on the device (temporal.hip), docs/SPEC.md §9: one fused pass that reprojects the history of the
// previous call to this call's pixels and blends the assembled frame into it. denoise_host.cpp owns the buffers (context.h TemporalHistory) and
// calls it between the guide pass and the à-trous passes. A call that uses the geometry snapshot of PT_TEMPORAL_MOTION (§9.1) launches
// the motion kernel instead.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include "../../include/ptrt.h"

namespace ptrt {

// §9 defaults, the exact f32 values SPEC §9 states
constexpr uint32_t kTemporalMaxHistory = 32u, kTemporalMaxHistoryLimit = 1048576u;
constexpr float kTemporalPlaneTolerance = 0x1p-7f, kTemporalNormalMin = 0.875f;

struct TemporalArgs {
    pt_camera cam, old_cam;       // this call's camera and the history's (the launcher clears both jitter words: §8.1 / §9 rays)
    uint32_t width, height;
    bool has_history;             // false: every pixel is out = c, l = 1 (the old_* planes are not read)
    bool same_camera;             // the 16 words of the two cameras are equal: one tap at the pixel itself
    bool match_ids;               // PT_TEMPORAL_MATCH_IDS
    float max_history;            // (float)max_history, resolved
    float tau_p2;                 // tau_p * tau_p, resolved
    float tau_n;                  // resolved
    const float4 *frame, *g0, *g1;            // this call's frame and guides
    const float4 *old_g0, *old_g1, *old_h;    // the history: guides, accumulated rgb | length
    float4 *out;                  // accumulated rgb | the frame's alpha (what is handed out and filtered)
    float4 *new_h;                // accumulated rgb | length (the next history)
    uint32_t *taken;              // kTemporalCounters counters, 16 words (one 64-B line) apart, zeroed by the caller: their sum += pixels
                                  // with l > 1 (one atomic per wave that has any)
};
constexpr uint32_t kTemporalCounters = 64u;
constexpr uint32_t kTemporalCounterWords = kTemporalCounters * 16u; // what `taken` points at
// All planes are width x height row-major; out and new_h must not alias any plane that is read.
hipError_t launch_temporal(hipStream_t s, const TemporalArgs &a);

// §9.1: what the motion pass reads besides TemporalArgs. The scene's arrays are those the guides of this call were traced on; the
// snapshot arrays hold the same primitives as the previous call saw them.
struct MotionArgs {
    const uint32_t *blob_of;      // original triangle id -> blob index (CommitCaches::d_blob_of), n_tris entries
    const float4 *tris;           // DeviceScene::tris: the 64-B records
    const float4 *spheres;        // DeviceScene::spheres
    const float *snap_tris;       // 9 floats per triangle by original id
    const float4 *snap_spheres;   // centre | radius per sphere
    uint32_t n_tris, n_spheres;   // original triangles (ids below n_tris), spheres (ids from n_tris on)
    uint32_t *moved;              // counter lines like `taken`, zeroed by the caller: their sum += hit pixels whose primitive moved
};
// a.has_history must hold (a call without a history has nothing to reproject: launch_temporal)
hipError_t launch_temporal_motion(hipStream_t s, const TemporalArgs &a, const MotionArgs &m);

} // namespace ptrt
