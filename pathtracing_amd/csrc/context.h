// context.h — pt_context, and one owner each for what a context keeps between public calls: the assembled frame with the results
// denoised and displayed from it, the history of pt_denoise_temporal, the exposure pt_display adapts from, the partial sums a PT_FLAG_ACCUMULATE frame continues, the frame-start template, the queue sizes a frame's loops
// read back, and the plumbing of a ray query. Each owner keeps its validity private and offers the few questions and transitions the
// calls need; nobody else keeps a flag about it. Private to api.cpp, frame.cpp, query.cpp, denoise_host.cpp,
// display_host.cpp and scene.cpp, as are the helpers every public call uses (defined once, in api.cpp).
#pragma once
#include "ptrt_internal.h"
#include "device_owner.h"
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

namespace ptrt {

pt_status fail(pt_context *ctx, pt_status code, const char *fmt, ...); // sets the context's (NULL: the thread's) last error, returns code
#define HIP_TRY(ctx, expr)                                                                          \
    do { hipError_t _e = (expr);                                                                    \
         if (_e != hipSuccess)                                                                      \
             return fail(ctx, _e == hipErrorOutOfMemory ? PT_ERR_OUT_OF_MEMORY : PT_ERR_HIP,        \
                         "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

void context_drain(pt_context *c); // nothing of the context's may still run: on its loop streams or its own

// The public half of a call that enqueues work: an error exit may leave kernels or copies in flight (on the loop streams too), and nothing
// of a failed call runs on after it
template <typename Call> pt_status drained_on_failure(pt_context *c, Call call)
{
    const pt_status st = call();
    if (st != PT_OK && c) { (void)hipSetDevice(context_device(c)); context_drain(c); }
    return st;
}

// A caller's device array must lie inside one allocation on the context's device: the kernel reads / writes `bytes` from `p` unchecked.
pt_status check_device_array(pt_context *c, const void *p, uint64_t bytes, const char *what, const char *who = "pt_trace_rays",
                             const char *host_flag = "PT_TRACE_HOST_MEMORY");

pt_status layout_of(const pt_render_params *p, pt_tile_layout *o); // pt_tile_layout_query without the error text
// The body of every copy-out call: `need` elements of `elem` bytes each from `src` on the device to the caller's `have` elements, then wait
pt_status copy_out(pt_context *c, void *dst, const void *src, uint64_t need, size_t elem, uint64_t have, const char *unit);

constexpr uint32_t kLag = 5; // most wavefront iterations kept in flight before the host looks at a queue size (ring sizes; pt_tuning.lag)
constexpr uint32_t kRingWords = kShards * kCounterStride; // one iteration's readback: (up to) the kShards extend-queue sizes
constexpr uint32_t kMaxGroups = 4;  // independent wavefront loops (shard groups) per frame, each on its own stream

// A host copy of counter words [first, ...) of a counter block (ptrt_internal.h kCnt*), addressed by the block's own word indices
struct CounterView {
    const uint32_t *words; uint32_t first;
    uint32_t word(uint32_t w) const { return words[w - first]; }
    uint64_t u64(uint32_t w) const { return (uint64_t)word(w) | ((uint64_t)word(w + 1) << 32); }
    uint32_t error() const { return word(kCntError); } // 1 = traversal stack overflow, 2 = step limit
};

// What a context hands out: the assembled frame (float and UNORM8), this rank's tile block, what pt_denoise made of the frame
// (docs/SPEC.md §8: guide rays in dn_work — 2 rows per pixel; then the filter's two ping-pong images —, their hits, the two guide planes and
// the denoised image) and what pt_display made of it (§10). The denoised and displayed results are results of the frame the framebuffer
// holds: they have its size, and they go when a call begins to replace it.
class FrameOutputs {
public:
    enum class Holds { nothing, path_traced, reference_sphere };
    DevBuf<float4> fb, tiles;
    DevBuf<uint32_t> fb8;
    DevBuf<float4> dn_work, dn_hits, dn_g0, dn_g1, dn_out;
    DevBuf<float4> tm_out;           // pt_denoise_temporal: accumulated rgb | the frame's alpha
    Event ev_denoise[3];             // start, guides done, filter done (made by the first pt_denoise)
    Event ev_temporal;               // temporal pass done (made by the first pt_denoise_temporal)
    DevBuf<uint32_t> disp8;          // pt_display: one R | G<<8 | B<<16 | A<<24 word per pixel
    DevBuf<uint32_t> disp_meter;     // its 512 histogram words, then its pt_display_info (display.h kDisplayMeterWords)
    Event ev_display[3];             // start, metering done, tone pass done (made by the first pt_display)

    hipError_t resize(uint32_t width, uint32_t height)
    {
        const size_t n = (size_t)width * height;
        hipError_t e = fb.ensure(n);
        if (e == hipSuccess) e = fb8.ensure(n);
        if (e == hipSuccess) { w = width; h = height; }
        return e;
    }
    uint32_t width() const { return w; }
    uint32_t height() const { return h; }
    uint64_t pixels() const { return (uint64_t)w * h; }

    void replace() { holds_ = Holds::nothing; drop_denoised(); temporal_ = false; displayed_ = false; } // this call replaces the frame: nothing of the old one is handed out any more
    // A pt_render that failed: no frame. (Stale-looking and pinned, tests/test_gpu_context_state.py: a call refused before it began to
    // replace the frame — params == NULL, a bad size — ends here too, with the denoised results still readable.)
    void lost() { holds_ = Holds::nothing; }
    void complete(Holds kind) { holds_ = kind; }
    Holds holds() const { return holds_; }
    bool readable() const { return holds_ != Holds::nothing; }

    void drop_denoised() { guides_ = image_ = false; }      // pt_denoise rewrites its buffers from here on
    void denoised(bool with_image) { denoised(with_image, dn_g0.p, dn_g1.p); }
    void denoised(bool with_image, const float4 *g0, const float4 *g1) { guides_ = true; image_ = with_image; g0_ = g0; g1_ = g1; }
    bool has_guides() const { return guides_; }
    bool has_image() const { return image_; }
    void guides_from(const float4 *&g0, const float4 *&g1) const { g0 = g0_; g1 = g1_; } // the two planes has_guides() speaks of

    void drop_temporal() { temporal_ = false; }              // pt_denoise_temporal rewrites tm_out from here on
    void accumulated() { temporal_ = true; }
    bool has_temporal() const { return temporal_; }

    void drop_display() { displayed_ = false; }              // pt_display rewrites disp8 and disp_meter from here on
    void displayed() { displayed_ = true; }
    bool has_display() const { return displayed_; }

    // The tile block outlives the frame: after a reference-sphere or a failed frame it is still the last path-traced frame's (pinned too).
    void tiles_hold(uint32_t pixel_slots) { tile_slots_ = pixel_slots; }
    uint32_t tile_slots() const { return tile_slots_; }

private:
    uint32_t w = 0, h = 0, tile_slots_ = 0;
    Holds holds_ = Holds::nothing;
    bool guides_ = false, image_ = false, temporal_ = false, displayed_ = false;
    const float4 *g0_ = nullptr, *g1_ = nullptr;
};

// What pt_denoise_temporal keeps between calls (docs/SPEC.md §9): the previous successful call's guides, its accumulated colour with the
// history length in .w, its camera and its size. Two sets of planes: a call reads the front set and writes the back set, and only
// commit() — the last thing a successful call does — makes the back set the history, so a call that fails on the way leaves the history
// as it was, and pt_denoise (which writes FrameOutputs' own guide planes) never touches it. Kept across frames, queries and geometry
// updates; dropped by drop(), by a size change and with the context.
// With PT_TEMPORAL_MOTION (§9.1) a set also holds the geometry its call was traced on — every triangle's 9 floats by original id, every
// sphere's 4 — and which scene state that was (SceneState). The snapshot goes the way of the planes: written to the back set, current
// after commit(), and gone after a commit() without one.
class TemporalHistory {
public:
    struct Planes { const float4 *g0, *g1, *h; };
    struct Target { float4 *g0, *g1, *h; };
    struct SceneState { uint64_t serial, updates; uint32_t n_tris, n_spheres; }; // pt_scene's serial and update count, its primitive counts
    struct Snapshot { const float *tris; const float4 *spheres; };
    struct SnapshotTarget { float *tris; float4 *spheres; };
    DevBuf<uint32_t> taken;          // counter lines of the call under way: pixels that took history (temporal.h)
    DevBuf<uint32_t> moved;          // §9.1's second set of lines: hit pixels whose primitive moved (made by the first flagged call)

    // the planes of a w x h call; a history of another size is dropped (its planes may be reallocated)
    hipError_t reserve(uint32_t width, uint32_t height, size_t counter_words)
    {
        if (width != w_ || height != h_) valid_ = false;
        const size_t n = (size_t)width * height;
        for (auto &set : sets_)
            for (auto *b : { &set.g0, &set.g1, &set.h })
                if (const hipError_t e = b->ensure(n)) { valid_ = false; return e; }
        return taken.ensure(counter_words);
    }
    // the back set's snapshot arrays for a scene of these counts (the front set's stay as they are: a failed call leaves them readable)
    hipError_t reserve_snapshot(const SceneState &of, size_t counter_words)
    {
        Set &s = sets_[cur_ ^ 1u];
        if (const hipError_t e = s.snap_tris.ensure((size_t)of.n_tris * 9u)) return e;
        if (const hipError_t e = s.snap_spheres.ensure(of.n_spheres)) return e;
        return moved.ensure(counter_words);
    }
    bool matches(uint32_t width, uint32_t height) const { return valid_ && width == w_ && height == h_; }
    const pt_camera &camera() const { return cam_; }
    Planes front() const { const Set &s = sets_[cur_]; return Planes{ s.g0.p, s.g1.p, s.h.p }; }
    Target back() { Set &s = sets_[cur_ ^ 1u]; return Target{ s.g0.p, s.g1.p, s.h.p }; }
    // the history's snapshot was recorded from this scene (same serial: same object, no commit since)
    bool snapshot_of(const SceneState &now) const
    {
        const Set &s = sets_[cur_];
        return s.has_snapshot && s.state.serial == now.serial && s.state.n_tris == now.n_tris && s.state.n_spheres == now.n_spheres;
    }
    bool snapshot_is_current(const SceneState &now) const { return sets_[cur_].state.updates == now.updates; } // no update has run since
    Snapshot snapshot() const { const Set &s = sets_[cur_]; return Snapshot{ s.snap_tris.p, s.snap_spheres.p }; }
    SnapshotTarget snapshot_back() { Set &s = sets_[cur_ ^ 1u]; return SnapshotTarget{ s.snap_tris.p, s.snap_spheres.p }; }
    // `recorded`: the state the back set's snapshot was copied at, or NULL for a call without PT_TEMPORAL_MOTION (no snapshot stays)
    void commit(const pt_camera &cam, uint32_t width, uint32_t height, const SceneState *recorded = nullptr)
    {
        cur_ ^= 1u; cam_ = cam; w_ = width; h_ = height; valid_ = true;
        sets_[cur_].has_snapshot = recorded != nullptr;
        if (recorded) sets_[cur_].state = *recorded;
    }
    void drop() { valid_ = false; }

private:
    struct Set { DevBuf<float4> g0, g1, h; DevBuf<float> snap_tris; DevBuf<float4> snap_spheres; SceneState state{}; bool has_snapshot = false; };
    Set sets_[2];
    uint32_t cur_ = 0, w_ = 0, h_ = 0;
    pt_camera cam_{};
    bool valid_ = false;
};

// What pt_display keeps between calls (docs/SPEC.md §10): one f32 on the device, the last adapted exposure E_a. Two slots, as the temporal
// history has two sets of planes: a metering call reads the front slot (when there is a state) and its resolve kernel writes the back
// slot; only commit() — after the call's final synchronise succeeded — makes that the state, so a call that fails leaves it as it was.
// Kept across every other call; dropped by drop() and with the context. Calls without PT_DISPLAY_AUTO_EXPOSURE never look at it.
class DisplayAdaptation {
public:
    hipError_t reserve() { return slots_.ensure(2); }
    bool valid() const { return valid_; }
    const float *front() const { return slots_.p + cur_; }
    float *back() { return slots_.p + (cur_ ^ 1u); }
    void commit() { cur_ ^= 1u; valid_ = true; }
    void drop() { valid_ = false; }

private:
    DevBuf<float> slots_;
    uint32_t cur_ = 0;
    bool valid_ = false;
};

// What the partial sums in pt_context::acc hold, for PT_FLAG_ACCUMULATE to continue: the frame geometry they were made with, whether they
// are next-event estimates (the two kinds of sum do not mix), and the samples so far. Invalid from begin() until complete().
class Accumulation {
public:
    struct Key { uint32_t w, h, rank, nranks, streams, seed; bool nee; bool spheres = false; }; // spheres: PT_FLAG_NEXT_EVENT_SPHERES (docs/SPEC.md §7.1)
    enum class Refusal { none, other_frame, other_estimator, other_light_set, wrong_offset };
    Refusal continues(const Key &k, uint32_t sample_offset) const
    {
        if (spp == 0 || key.w != k.w || key.h != k.h || key.rank != k.rank || key.nranks != k.nranks || key.streams != k.streams || key.seed != k.seed)
            return Refusal::other_frame;
        if (key.nee != k.nee) return Refusal::other_estimator;
        if (key.spheres != k.spheres) return Refusal::other_light_set;
        return sample_offset != spp ? Refusal::wrong_offset : Refusal::none;
    }
    uint64_t samples() const { return spp; }
    bool next_event() const { return key.nee; }
    bool sphere_lights() const { return key.spheres; }
    void begin() { spp = 0; }
    void complete(const Key &k, uint64_t total_spp) { key = k; spp = total_spp; }

private:
    Key key{};
    uint64_t spp = 0;
};

// Queue sizes on their way to the host, kLag iterations deep for each of the kMaxGroups loops, in one of two modes (pt_tuning.readback,
// fixed per frame by begin()): mapped — the extend kernels store the lines to host-mapped pinned memory themselves (PathState::host_ring;
// launch j + 1 writes iteration j's) — or one 2-4 KB copy per launch. Which event to wait for, where an iteration's lines are and how far
// apart is known here and nowhere else. The pinned block of the copy mode has two more regions, for the two other small synchronous
// reads of a frame: all counters at the frame's end, and the shard sizes of a dense frame-start template.
class QueueSizes {
public:
    struct Sizes { uint32_t longest; uint64_t alive, traced; }; // over a loop's shards: longest queue (holes included), alive entries, rays traced
    hipError_t alloc() // can_map() is false afterwards on a platform without host-mapped pinned memory: copy mode only
    {
        const hipError_t e = h_counts.alloc(kTemplateOffset + kRingWords);
        if (e == hipSuccess && h_ring.alloc(kLag * kShards, true) == hipSuccess) std::memset(h_ring.p, 0, sizeof(uint4) * kLag * kShards);
        else if (e == hipSuccess) (void)hipGetLastError();
        return e;
    }
    hipError_t create_events()
    {
        for (auto &row : ev_lag) for (auto &ev : row) if (const hipError_t e = ev.create(false)) return e;
        return hipSuccess;
    }
    bool can_map() const { return h_ring.d != nullptr; }
    uint4 *begin(bool mapped) { mapped_ = mapped; return mapped ? h_ring.d : nullptr; } // a frame starts: what PathState::host_ring is to be
    uint32_t *frame_end() const { return h_counts.p + kFinalOffset; }           // kCntTotalWords
    uint32_t *template_sizes() const { return h_counts.p + kTemplateOffset; }   // kRingWords

    // after loop g's launch `it` on `stream`: the lines of the queue it filled — `n_shards` from `lines` on, in the device's counter block
    hipError_t post(hipStream_t stream, uint32_t g, uint32_t it, const uint32_t *lines, uint32_t n_shards)
    {
        const uint32_t ring = it % kLag;
        if (!mapped_) {
            const hipError_t e = hipMemcpyAsync(copied(g, ring), lines, sizeof(uint32_t) * n_shards * kCounterStride, hipMemcpyDeviceToHost, stream);
            if (e != hipSuccess) return e;
        }
        return hipEventRecord(ev_lag[g][ring], stream);
    }
    // what iteration `old_it` of loop g (shards first_shard .. + n_shards) left; at most kLag - 1 iterations have been posted since
    hipError_t wait(uint32_t g, uint32_t old_it, uint32_t first_shard, uint32_t n_shards, Sizes &out)
    {
        // mapped: launch old_it + 1 stored old_it's lines (fold_traced); it is at most the launch just enqueued since lag >= 2
        const hipError_t e = hipEventSynchronize(ev_lag[g][(mapped_ ? old_it + 1u : old_it) % kLag]);
        if (e != hipSuccess) return e;
        const volatile uint32_t *h_old = mapped_ ? (const volatile uint32_t *)(h_ring.p + (size_t)(old_it % kLag) * kShards + first_shard)
                                                 : copied(g, old_it % kLag);
        // a shard's line: word 0 = queue length (holes included), word 1 = alive entries, words 2-3 = rays the iteration traced
        const uint32_t line = mapped_ ? 4u : kCounterStride;
        out = Sizes{ 0u, 0u, 0u };
        for (uint32_t sh = 0; sh < n_shards; ++sh) {
            out.longest = std::max(out.longest, (uint32_t)h_old[sh * line]);
            out.alive += h_old[sh * line + 1];
            out.traced += (uint64_t)h_old[sh * line + 2] | ((uint64_t)h_old[sh * line + 3] << 32);
        }
        return hipSuccess;
    }

private:
    static constexpr size_t kFinalOffset = (size_t)kMaxGroups * kLag * kRingWords;
    static constexpr size_t kTemplateOffset = kFinalOffset + kCntTotalWords;
    uint32_t *copied(uint32_t g, uint32_t ring) const { return h_counts.p + ((size_t)g * kLag + ring) * kRingWords; }
    Pinned<uint32_t> h_counts;    // copy mode: kLag readbacks of the per-shard queue sizes per loop; then the two regions above
    Pinned<uint4> h_ring;         // mapped: kLag x kShards lines (.p host address, .d device address)
    Event ev_lag[kMaxGroups][kLag];
    bool mapped_ = false;
};

// What k_generate would write at the start of every frame of a fused pipeline, kept from the first frame of its kind: the first
// extend queue (every shard's slots in slot order, holes for off-image pixels and sample-less streams) and the counter block
// that goes with it. A frame then starts with one 2.4 KB device copy instead of a kernel over every slot; the first extend
// launch reads the template in place of q_ext[0] and zeroes the radiance sums of the slots it starts (kernels.hip, it == 0).
// Invariant: a template may start a non-accumulate frame only if every `acc` slot its first queue does not start holds zero. A template in
// which every stream has a sample starts every in-image slot (off-image slots are never written). A dense one (first_spp < streams) leaves
// whole streams out: the non-accumulate frame that builds it zeroes them, and frame_ran() drops it after any other kind of frame, since
// accumulate frames keep those streams' sums and full-state frames start every stream.
class FrameTemplate {
public:
    struct Key { uint32_t w, h, rank, nranks, streams, first_spp, offset, n_slots, shard_cap, pad; const void *q, *acc; // q: filled in here
                 bool operator==(const Key &o) const { return std::memcmp(this, &o, sizeof *this) == 0; } }; // (no padding: pad is 0)
    hipError_t reserve(size_t q_entries)
    {
        const hipError_t e = q_init.ensure(q_entries);
        return e != hipSuccess ? e : cnt_init.ensure(kCntTotalWords);
    }
    // Build it on `q` if this key differs from the one it was built for (frame.cpp); `sizes` lends the host block for a dense template's bound
    pt_status build_if_differs(pt_context *c, hipStream_t q, Key key, const Pipeline &pipe, const DeviceScene &ds, const PathState &ps,
                               const FrameParams &fp, const QueueSizes &sizes);
    void frame_ran(bool accumulate_or_full_state) { if (accumulate_or_full_state && key_.first_spp < key_.streams) valid = false; }
    const uint32_t *counters() const { return cnt_init.p; }   // what the frame's counter block starts as
    uint32_t *first_queue() const { return q_init.p; }        // what the frame's first launch reads: read, never written
    uint32_t first_bound() const { return bound; }            // longest shard queue of the template: the first launch's grid bound

private:
    DevBuf<uint32_t> q_init, cnt_init;
    Key key_{};
    bool valid = false;
    uint32_t bound = 0;
};

// The plumbing of a query (pt_trace_rays, pt_gather, pt_gather_paths, pt_denoise's guide pass): its own counter block, overflow stack, staging buffers
// (PT_TRACE_HOST_MEMORY) and events, so that a query touches nothing a frame reads (the frame-start template, the partial sums, the queues
// and their counters). All on the context's stream (query.cpp; the guide pass is denoise_host.cpp's).
class Queries {
public:
    DevBuf<float4> rays, hits;       // staging
    Event ev[2];
    struct Counts { uint32_t error; uint64_t node_visits, tri_tests, sphere_tests; };
    // sizes the overflow area (`overflow` stack entries per ray beyond those in LDS) for launches of up to n_rays rays, zeroes the counter
    // words the kernels use and fills the fields of `ps` that launch_trace reads
    pt_status setup(pt_context *c, uint32_t overflow, uint64_t n_rays, PathState &ps);
    pt_status launch(pt_context *c, const DeviceScene &ds, const PathState &ps, const float4 *rays, float4 *hits, uint64_t n_rays, bool occlusion, bool count);
    // copies those words back, waits for the stream (and with it for everything the caller enqueued) and reads them
    pt_status finish(pt_context *c, Counts &out);

private:
    DevBuf<uint32_t> cnt;
    DevBuf<int32_t> ovf;
};

} // namespace ptrt

// Every device buffer, event, stream and pinned block below is an owner of device_owner.h: declaring it here is all it takes, the destructor
// gives it back. pt_context_destroy drains the streams in its body before any member goes, so the order of the members is free.
struct pt_context {
    int device = 0;
    ptrt::Stream stream;            // pt_device_desc::stream (borrowed) or the context's own
    std::string err;
    // path state
    ptrt::DevBuf<float4> ray_o, ray_d, thr, acc;
    ptrt::DevBuf<float4> nee_ext, nee_rad; // PT_FLAG_NEXT_EVENT frames only: a slot's pending shadow ray (ptrt_internal.h NeeArgs)
    ptrt::DevBuf<float2> hit;       // split frames only (k_shade reads what the extend kernel found), like the two specular buckets
    ptrt::DevBuf<uint32_t> sd, q_ext0, q_ext1, q_metal, q_dielectric, counters;
    ptrt::DevBuf<int32_t> stack_ovf;
    ptrt::Accumulation sums;        // what `acc` holds
    ptrt::FrameTemplate start;
    ptrt::QueueSizes sizes;
    ptrt::Stream group_stream[ptrt::kMaxGroups]; // group 0 runs on `stream` when there is one group only
    ptrt::Event ev_fork, ev_join[ptrt::kMaxGroups];
    pt_tuning tuning = { // the scheduling knobs (include/ptrt.h): defaults and the measurements behind them
        0,    // bounces (1..64): path vertices per launch of the fused kernel (state in registers); 0 = 3/4 max_depth - 2 clamped to
              // [4, 12]: depth 8 -> 4, depth 16 -> 10 (ms per frame with 2 / 3 / 4 / 6 / 8 / 12 vertices: 1M-triangle Cornell, depth 8:
              // 18.57 / 17.80 / 17.52 / 17.50 / 17.68 / 17.87; Cornell+glass+metal, depth 16: 47.5 / 41.0 / 38.3 / 35.3 / 34.3 / 33.5)
        0,    // loops (1, 2, 4) overrides; 0 = two loops, whose launch tails overlap. Measured (tools/exp_loops.py, ms per frame with
              // 1 / 2 / 4 loops): 1M-tri Cornell 1080p/64spp 18.42 / 18.08 / 18.77, a rank's 1/8 of it 4.11 / 3.81 / -, soup 76.2 / 73.3 /
              // 72.3, glass 256 spp 37.8 / 37.0 / 36.6, 4K/1024 spp 1062 / 1051 / 1046. Frames that time single kernels
              // (PT_FLAG_PROFILE_KERNELS, visit counting, the extend-kernel probe) run one loop, so that a timed launch has the GPU to itself.
        4096, // finish_below: a shard with no more alive paths than this runs them to their end in one launch of the fused kernel (0 = never)
        0,    // packed_chunk: queue entries per wavefront of the lane-packing kernel (0 = by stream count)
        0.9f, // compact_below: a shard re-packs its queue in a launch that would leave alive/length below this (>1 = every launch, 0 = never); else carried in place (want_compact)
        0.f,  // sparse_below (0 = off, the default: measured ±0): see PathState::sparse_below
        32,   // sticky_samples. Measured, 1M-tri Cornell 1080p, ms per frame by spp (8 streams), start-of-launch ratio (round 1) / predicted ratio / sticky / every launch:
              //   8: 4.13/4.20/4.07/3.01  32: 10.95/10.93/9.70/9.61  64: 19.28/18.82/18.45/18.36  128: 38.15/36.12/36.04/36.06
              //   256: 73.06/71.95/71.99/72.15  512: 142.8/141.5/143.0/143.7  1024: 284.5/283.7/289.9/292.5; 4K/1024: 1067.7/1064.1/1097.0/1108 (tools/exp_compact.py)
        0,    // lag (2..5; 0 = by frame length, see plan_frame)
        0,    // extend_kernel: 0 = probed per scene (ExtendChoice), else the ExtendKernel every scene uses
        0,    // readback: 0 = the kernels store the sizes to host-mapped memory, 1 = one 2-4 KB copy per launch (pt_context_create falls back to it)
    };
    ptrt::Event ev_start, ev_stop;
    ptrt::Event ev_probe[4];           // brackets of the two probe iterations that pick the extend kernel
    std::vector<ptrt::Event> ev_pool;  // PT_FLAG_PROFILE_KERNELS: three per iteration, made when a frame first needs them (frame.cpp pool_event)
    ptrt::FrameOutputs out;
    ptrt::TemporalHistory history;
    ptrt::DisplayAdaptation adaptation;
    ptrt::Queries query;
};
