// api.cpp — C ABI of libptrt.so (include/ptrt.h): context, wavefront frame loop, ray queries, denoising, read-backs (scenes: scene.cpp).
// Stands where Renderer.CreateResources / CreateComputePipeline / ComputeFrame + the compute-fence wait stand in
// the reference (RayTracing/Graphics/Renderer.cs:105-196, 293-403, 1006-1040, 970-972).
// HIP only: there is no CPU fallback anywhere in this library.
#include "scene.h"
#include "denoise.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace ptrt;

namespace {

thread_local std::string g_err;

constexpr uint32_t kLag = 5; // most wavefront iterations kept in flight before the host looks at a queue size (ring sizes; pt_tuning.lag)
constexpr uint32_t kRingWords = kShards * kCounterStride; // one iteration's readback: (up to) the kShards extend-queue sizes
constexpr uint32_t kMaxGroups = 4;  // independent wavefront loops (shard groups) per frame, each on its own stream
constexpr size_t kFinalOffset = (size_t)kMaxGroups * kLag * kRingWords; // where the frame-end copy of all counters lands in h_counts

uint32_t host_pcg(uint32_t x)
{
    uint32_t s = x * 747796405u + 2891336453u;
    uint32_t w = ((s >> ((s >> 28) + 4u)) ^ s) * 277803737u;
    return (w >> 22) ^ w;
}

// Which extend kernel a frame runs. A frame's PT_FLAG_EXTEND_* beats pt_tuning.extend_kernel, which beats the scene's own choice, measured:
//   inside a frame : iteration 2 of group 0 runs the one-ray-per-lane kernel, iteration 3 the lane-packing one (bit-identical results), each
//                    bracketed by events; accepted only if both traced a real share of the frame's slots;
//   across frames  : a frame too short for that (few samples per stream: it is over in two iterations) runs whole on one kernel — the first
//                    on the one-ray-per-lane kernel, the next on the lane-packing one — and the rays per millisecond of the two frames decide.
// The faster per ray wins (packed needs +10 %). Deep incoherent traversals (1M-triangle soup) gain ~2.5x from packing, shallow ones (walls of
// a box) lose ~35 %, and no static property of the tree tells them apart. Counting / profiling frames neither probe nor feed
// the decision: their kernels are instrumented builds. A probing frame runs one loop and no finish mode, so that its timed iterations compare.
uint32_t faster(double rate_simple, double rate_packed) { return rate_packed > 1.10 * rate_simple ? EXT_PACKED : EXT_SIMPLE; }
struct ExtendFrame {            // the choice during one frame
    ExtendChoice &mem;
    bool undecided;             // nothing forces a kernel and the scene has not picked one: this frame measures (whole, on frame_kernel)
    uint32_t frame_kernel, kernel; // kernel: 0 = probing inside this frame, else the ExtendKernel every iteration uses
    bool mixed = false;         // this frame ran probe iterations on both kernels: its overall rate says nothing about either
    uint64_t probe_n[2] = { 0, 0 }; // rays traced by probe iterations 2 and 3
    ExtendFrame(ExtendChoice &m, uint32_t forced, bool instrumented) : mem(m),
        undecided(forced == 0u && m.kernel == 0u && !instrumented),
        frame_kernel((undecided && m.rate_simple > 0.0 && m.rate_packed == 0.0) ? EXT_PACKED : EXT_SIMPLE), // first the default, then the other
        kernel(forced ? forced : m.kernel ? m.kernel : (undecided && frame_kernel == EXT_SIMPLE) ? 0u : frame_kernel) {}
    bool probing(uint32_t g, uint32_t it) const { return g == 0u && kernel == 0u && (it == 2u || it == 3u); }
    int launch_kernel(uint32_t g, uint32_t it, bool split) const { return (kernel == EXT_PACKED || (probing(g, it) && it == 3u)) ? EXT_PACKED : (kernel == EXT_POOL && !split) ? EXT_POOL : EXT_SIMPLE; }
    // default path vertices per launch. Lane-packing: a lane pulls a new entry whenever its budget ends, so a long budget costs nothing and saves
    // launches (ms per frame with 8 / 16 / 32 / 64 vertices, tools/exp_packed.py: 1M soup 72.2 / 71.5 / 70.5 / 67.4, at 256 spp 277.6 / 271.8 /
    // 268.3 / 266.1, 5k soup 7.99 / 7.43 / 7.35 / 7.39); the probe iteration keeps 8 so that it stays comparable with the one before it
    uint32_t bounces(uint32_t g, uint32_t it, int k, uint32_t simple) const { return k != EXT_PACKED ? simple : probing(g, it) ? 8u : 64u; }
    // loop g's readback of iteration `it`, which traced `traced` rays; by iteration 3's, both probe iterations and their events `ev` (start and
    // end of each, pt_context::ev_probe) are complete
    hipError_t observe(uint32_t g, uint32_t it, uint64_t traced, uint32_t loop_slots, const Event *ev)
    {
        if (!probing(g, it)) return hipSuccess;
        probe_n[it - 2u] = traced;
        if (it == 2u) return hipSuccess;
        float ms_simple = 0.f, ms_packed = 0.f; hipError_t e = hipEventElapsedTime(&ms_simple, ev[0], ev[1]);
        if (e != hipSuccess || (e = hipEventElapsedTime(&ms_packed, ev[2], ev[3])) != hipSuccess) return e;
        const uint64_t enough = (uint64_t)loop_slots / 8u; // each probe iteration must have traced a real share of the slots
        if (probe_n[0] < enough || probe_n[1] < enough) { // inconclusive (the frame was all but over): finish on the default, whole frames decide
            kernel = EXT_SIMPLE; mixed = probe_n[1] >= enough / 8u; // did the lane-packing iteration trace enough to colour this frame's rate?
        } else kernel = mem.kernel = faster(probe_n[0] / std::max((double)ms_simple, 1e-6), probe_n[1] / std::max((double)ms_packed, 1e-6));
        return hipSuccess;
    }
    // the whole frame: a warm one (cold = it had to allocate: first touch of fresh memory is 30 % slower, not a measurement) on one
    // kernel of at least 2^20 rays gives that kernel's rate
    void frame_done(uint64_t rays, double gpu_ms, bool cold)
    {
        if (!undecided || mem.kernel != 0u || cold) return;
        if (mixed || rays < (1u << 20) || !(gpu_ms > 0.0)) { if (++mem.misses >= 3u) mem.kernel = EXT_SIMPLE; return; }
        (frame_kernel == EXT_PACKED ? mem.rate_packed : mem.rate_simple) = (double)rays / gpu_ms;
        if (mem.rate_simple > 0.0 && mem.rate_packed > 0.0) mem.kernel = faster(mem.rate_simple, mem.rate_packed);
    }
};

} // namespace

// Every device buffer, event, stream and pinned block below is an owner of device_owner.h: declaring it here is all it takes, the destructor
// gives it back. pt_context_destroy drains the streams in its body before any member goes, so the order of the members is free.
struct pt_context {
    int device = 0;
    Stream stream;                  // pt_device_desc::stream (borrowed) or the context's own
    std::string err;
    // path state
    DevBuf<float4> ray_o, ray_d, thr, acc, tiles, fb;
    // what the partial sums in `acc` currently hold (PT_FLAG_ACCUMULATE continues them): frame geometry and samples so far
    uint32_t acc_w = 0, acc_h = 0, acc_rank = 0, acc_nranks = 0, acc_streams = 0, acc_seed = 0;
    uint64_t acc_spp = 0;
    bool acc_nee = false;           // ... and whether they are next-event estimates (PT_FLAG_NEXT_EVENT): the two do not mix
    DevBuf<float4> nee_ext, nee_rad; // PT_FLAG_NEXT_EVENT frames only: a slot's pending shadow ray (ptrt_internal.h NeeArgs)
    DevBuf<float2> hit;             // split frames only (k_shade reads what the extend kernel found), like the two specular buckets
    DevBuf<uint32_t> sd, q_ext0, q_ext1, q_metal, q_dielectric, counters, fb8;
    DevBuf<int32_t> stack_ovf;
    // What k_generate would write at the start of every frame of a fused pipeline, kept from the first frame of its kind: the first
    // extend queue (every shard's slots in slot order, holes for off-image pixels and sample-less streams) and the counter block
    // that goes with it. A frame then starts with one 2.4 KB device copy instead of a kernel over every slot; the first extend
    // launch reads q_init in place of q_ext[0] and zeroes the radiance sums of the slots it starts (kernels.hip, it == 0).
    // Invariant: a template may start a non-accumulate frame only if every `acc` slot its first queue does not start holds zero. A template in
    // which every stream has a sample starts every in-image slot (off-image slots are never written). A dense one (first_spp < streams) leaves
    // whole streams out: the non-accumulate frame that builds it zeroes them, and start_frame drops it after any other kind of frame, since
    // accumulate frames keep those streams' sums and full-state frames start every stream.
    DevBuf<uint32_t> q_init, cnt_init;
    struct InitKey { uint32_t w, h, rank, nranks, streams, first_spp, offset, n_slots, shard_cap; const void *q, *acc;
                     bool operator==(const InitKey &o) const { return std::memcmp(this, &o, sizeof *this) == 0; } } init_key{};
    bool init_valid = false;
    uint32_t init_bound = 0; // longest shard queue of the template: the first launch's grid bound
    Pinned<uint32_t> h_counts;    // kLag readbacks of the per-shard queue sizes (pt_tuning.readback = 1) + one copy of all counters
    Pinned<uint4> h_ring;         // mapped: the extend kernels report their queue sizes to it, kLag x kShards lines (.p host address, .d device
                                  // address; PathState::host_ring)
    Event ev_lag[kMaxGroups][kLag];
    Stream group_stream[kMaxGroups]; // group 0 runs on `stream` when there is one group only
    Event ev_fork, ev_join[kMaxGroups];
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
        0,    // readback: 0 = the kernels store the sizes to h_ring, 1 = one 2-4 KB copy per launch (pt_context_create falls back to it)
    };
    Event ev_start, ev_stop;
    Event ev_probe[4];           // brackets of the two probe iterations that pick the extend kernel
    std::vector<Event> ev_pool;  // PT_FLAG_PROFILE_KERNELS: three per iteration, made when a frame first needs them (pool_event)
    uint32_t fb_w = 0, fb_h = 0;
    uint32_t n_slots = 0; // slots of the last path-traced frame (acc layout)
    bool fb_valid = false;
    // pt_trace_rays: its own counter block, overflow stack, staging buffers (PT_TRACE_HOST_MEMORY) and events, so that a query touches
    // nothing a frame reads (the frame-start template, the partial sums, the queues and their counters)
    DevBuf<uint32_t> trace_cnt;
    DevBuf<int32_t> trace_ovf;
    DevBuf<float4> trace_rays, trace_hits;
    Event ev_trace[2];
    bool fb_reference = false;       // the framebuffer holds a PT_REFERENCE_SPHERE frame (pt_denoise refuses it)
    // pt_denoise (docs/SPEC.md §8): guide rays (2 rows per pixel; then the filter's two ping-pong images), their hits, the two guide
    // planes and the denoised image of a dn_w x dn_h framebuffer. dn_guides / dn_image: what the read functions may hand out (until the
    // next pt_render or pt_assemble_tiles)
    DevBuf<float4> dn_work, dn_hits, dn_g0, dn_g1, dn_out;
    uint32_t dn_w = 0, dn_h = 0;
    bool dn_guides = false, dn_image = false;
    Event ev_denoise[3];             // start, guides done, filter done (made by the first pt_denoise)
};

namespace {

pt_status layout_of(const pt_render_params *p, pt_tile_layout *o)
{
    if (!p || !o) return PT_ERR_INVALID_ARGUMENT;
    if (p->width == 0 || p->height == 0 || p->width > 32768 || p->height > 32768) return PT_ERR_INVALID_ARGUMENT;
    if (p->tile_size != 0 && p->tile_size != kTile) return PT_ERR_UNSUPPORTED;
    const uint32_t nr = p->nranks ? p->nranks : 1u;
    if (p->rank >= nr) return PT_ERR_INVALID_ARGUMENT;
    o->tile_size = kTile;
    o->tiles_x = (p->width + kTile - 1) / kTile;
    o->tiles_y = (p->height + kTile - 1) / kTile;
    o->n_tiles = o->tiles_x * o->tiles_y;
    o->tiles_mine = (o->n_tiles > p->rank) ? (o->n_tiles - p->rank + nr - 1) / nr : 0u;
    o->tiles_per_rank = (o->n_tiles + nr - 1) / nr;
    o->floats_per_tile = (uint64_t)kTilePixels * 4u;
    return PT_OK;
}

hipEvent_t pool_event(pt_context *c, size_t i)
{
    while (c->ev_pool.size() <= i) {
        Event e;
        if (e.create() != hipSuccess) return nullptr;
        c->ev_pool.push_back(std::move(e));
    }
    return c->ev_pool[i];
}

struct Frame {                  // a path-traced frame as plan_frame lays it out, and what its loops leave for finish_frame
    uint32_t nranks, streams, pixel_slots, n_slots, shard_cap, samples_per_stream, lag, n_loops, packed_chunk, default_bounces;
    uint32_t forced;            // ExtendKernel a frame flag or pt_tuning.extend_kernel forces (0 = none)
    bool profile, count, split, bucket, full_state, accumulate, mapped, compact;
    bool nee;                   // PT_FLAG_NEXT_EVENT (docs/SPEC.md §7): the one-ray-per-lane kernel with light samples
    NeeArgs nee_args;
    size_t q_entries; uint64_t total_spp, allocs_before;
    PathState ps; FrameParams fp;
    uint32_t iters; uint64_t slot_launches; size_t n_events; // launches of the longest loop, paths alive at launch starts, profile events
    std::vector<uint64_t> trace_alive, trace_rays;
};

} // namespace

namespace ptrt {
int context_device(const pt_context *c) { return c->device; }
hipStream_t context_stream(const pt_context *c) { return c->stream; }
void context_set_error(pt_context *c, const char *msg) { g_err = msg; if (c) c->err = msg; }
pt_status fail(pt_context *ctx, pt_status code, const char *fmt, ...)
{
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    context_set_error(ctx, buf);
    return code;
}
void context_drain(pt_context *c)
{
    for (auto &gs : c->group_stream) if (gs) (void)hipStreamSynchronize(gs);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
}
pt_status check_device_array(pt_context *c, const void *p, uint64_t bytes, const char *what, const char *who, const char *host_flag)
{
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess || (at.type != hipMemoryTypeDevice && !at.isManaged) || at.device != c->device) {
        (void)hipGetLastError();
        return fail(c, PT_ERR_INVALID_ARGUMENT, "%s: %s is not device memory of the context's device %d (host arrays: %s)", who, what, c->device, host_flag);
    }
    hipDeviceptr_t base = nullptr; size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) { (void)hipGetLastError(); return PT_OK; } // (range unknown: trust the caller)
    if ((const char *)p + bytes > (const char *)base + size)
        return fail(c, PT_ERR_INVALID_ARGUMENT, "%s: %s holds %llu bytes from the pointer on, the call needs %llu", who, what,
                    (unsigned long long)((const char *)base + size - (const char *)p), (unsigned long long)bytes);
    return PT_OK;
}
} // namespace ptrt

extern "C" {

uint32_t pt_abi_version(void) { return PTRT_ABI_VERSION; }

const char *pt_last_error(const pt_context *ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

pt_status pt_context_create(const pt_device_desc *desc, pt_context **out)
{
    if (!out) return fail(nullptr, PT_ERR_INVALID_ARGUMENT, "pt_context_create: out is NULL");
    *out = nullptr;
    const int dev = desc ? desc->device_ordinal : 0;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, PT_ERR_NO_DEVICE, "no HIP device visible (%s); libptrt has no CPU backend",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (dev < 0 || dev >= ndev) return fail(nullptr, PT_ERR_INVALID_ARGUMENT, "device ordinal %d out of range [0,%d)", dev, ndev);
    hipDeviceProp_t prop;
    HIP_TRY(nullptr, hipGetDeviceProperties(&prop, dev));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, PT_ERR_NO_DEVICE, "device %d is %s; libptrt ships gfx950 (MI355X) code objects only", dev, prop.gcnArchName);
    HIP_TRY(nullptr, hipSetDevice(dev));
    pt_context *c = new (std::nothrow) pt_context();
    if (!c) return fail(nullptr, PT_ERR_OUT_OF_MEMORY, "host allocation failed");
    c->device = dev;
    if (desc && desc->stream) c->stream.borrow((hipStream_t)desc->stream);
    else if ((e = c->stream.create()) != hipSuccess) { delete c; return fail(nullptr, PT_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e)); } // (the text this failure has always had)
    bool ok = c->h_counts.alloc(kFinalOffset + kCntTotalWords) == hipSuccess;
    // host-mapped ring for the kernels' own size reports; a platform without mapped pinned memory falls back to a copy per launch
    if (ok && c->h_ring.alloc(kLag * kShards, true) == hipSuccess) std::memset(c->h_ring.p, 0, sizeof(uint4) * kLag * kShards);
    else if (ok) { c->tuning.readback = 1u; (void)hipGetLastError(); }
    for (uint32_t g = 0; ok && g < kMaxGroups; ++g) ok = c->group_stream[g].create() == hipSuccess && c->ev_join[g].create(false) == hipSuccess;
    ok = ok && c->ev_fork.create(false) == hipSuccess && c->ev_start.create() == hipSuccess && c->ev_stop.create() == hipSuccess;
    for (auto &row : c->ev_lag) for (auto &ev : row) ok = ok && ev.create(false) == hipSuccess;
    for (auto &ev : c->ev_probe) ok = ok && ev.create() == hipSuccess;
    for (auto &ev : c->ev_trace) ok = ok && ev.create() == hipSuccess;
    ok = ok && c->counters.ensure(kCntTotalWords) == hipSuccess;
    if (!ok) { delete c; return fail(nullptr, PT_ERR_HIP, "context resource creation failed"); } // nothing runs yet: the owners give back what was made
    *out = c;
    return PT_OK;
}

pt_status pt_context_get_tuning(const pt_context *c, pt_tuning *o)
{
    if (!c || !o) return fail(nullptr, PT_ERR_INVALID_ARGUMENT, "pt_context_get_tuning: NULL argument");
    *o = c->tuning;
    return PT_OK;
}

pt_status pt_context_set_tuning(pt_context *c, const pt_tuning *t)
{
    if (!c || !t) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_context_set_tuning: NULL argument");
    if (t->bounces > 64) return fail(c, PT_ERR_INVALID_ARGUMENT, "tuning: bounces must be 0 (default) or 1..64");
    if (t->loops != 0 && t->loops != 1 && t->loops != 2 && t->loops != 4) return fail(c, PT_ERR_INVALID_ARGUMENT, "tuning: loops must be 0 (default), 1, 2 or 4");
    if (t->packed_chunk != 0 && (t->packed_chunk < 64 || t->packed_chunk > (1u << 20))) return fail(c, PT_ERR_INVALID_ARGUMENT, "tuning: packed_chunk must be 0 (default) or 64..2^20");
    if (t->lag != 0 && (t->lag < 2 || t->lag > kLag)) return fail(c, PT_ERR_INVALID_ARGUMENT, "tuning: lag must be 0 (default) or 2..%u", kLag);
    if (!(t->compact_below >= 0.f && t->compact_below <= 2.f) || !(t->sparse_below >= 0.f && t->sparse_below <= 1.f))
        return fail(c, PT_ERR_INVALID_ARGUMENT, "tuning: compact_below must be in [0,2], sparse_below in [0,1]");
    if (t->extend_kernel > (uint32_t)EXT_POOL) return fail(c, PT_ERR_INVALID_ARGUMENT, "tuning: extend_kernel must be 0 (probed), 1 (one ray per lane), 2 (lane-packing) or 3 (pooled)");
    if (t->readback > 1) return fail(c, PT_ERR_INVALID_ARGUMENT, "tuning: readback must be 0 (mapped store) or 1 (copy per launch)");
    if (t->readback == 0 && !c->h_ring.d) return fail(c, PT_ERR_UNSUPPORTED, "tuning: readback 0 needs host-mapped pinned memory, which this platform did not provide");
    c->tuning = *t; // all or nothing: a refused call changes no field
    return PT_OK;
}

void pt_context_destroy(pt_context *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    context_drain(c); // nothing may still run on what the members give back
    delete c;
}


void pt_scene_destroy(pt_scene *s) // (the scene's other calls: scene.cpp)
{
    if (!s) return;
    if (s->ctx) { (void)hipSetDevice(s->ctx->device); (void)hipStreamSynchronize(s->ctx->stream); }
    delete s;
}


// ------------------------------------------------------------------------------------------------ frame

pt_status pt_tile_layout_query(const pt_render_params *p, pt_tile_layout *o)
{
    pt_status st = layout_of(p, o);
    if (st != PT_OK) return fail(nullptr, st, "invalid render params for tile layout");
    return PT_OK;
}

static pt_status ensure_frame(pt_context *c, uint32_t w, uint32_t h)
{
    const size_t n = (size_t)w * h;
    HIP_TRY(c, c->fb.ensure(n));
    HIP_TRY(c, c->fb8.ensure(n));
    c->fb_w = w; c->fb_h = h;
    return PT_OK;
}

// Plan: validate, derive the frame's geometry and decoded flags, allocate what the frame uses, fill PathState and FrameParams
static pt_status plan_frame(pt_context *c, const pt_scene *s, const pt_render_params *p, const pt_tile_layout &lay, Frame &f)
{
    if (!s) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_render: scene is NULL");
    if (s->ctx != c) return fail(c, PT_ERR_INVALID_ARGUMENT, "scene belongs to another context");
    if (!s->committed) return fail(c, PT_ERR_NOT_COMMITTED, "scene not committed");
    if (p->spp == 0 || p->spp >= (1u << 24)) return fail(c, PT_ERR_INVALID_ARGUMENT, "spp must be in [1, 2^24)");
    if (p->max_depth == 0 || p->max_depth > 255) return fail(c, PT_ERR_INVALID_ARGUMENT, "max_depth must be in [1,255]");
    if (!std::isfinite(p->ray_eps) || p->ray_eps < 0.f) return fail(c, PT_ERR_INVALID_ARGUMENT, "ray_eps must be finite and >= 0");
    if (p->streams > 64) return fail(c, PT_ERR_INVALID_ARGUMENT, "streams must be in [0,64]");
    const pt_tuning &t = c->tuning;
    f.nranks = p->nranks ? p->nranks : 1u; f.streams = p->streams ? p->streams : 1u;
    f.pixel_slots = lay.tiles_per_rank * kTilePixels;                  // one slot per owned pixel ...
    const uint64_t slots64 = (uint64_t)f.pixel_slots * f.streams;      // ... per sample stream
    if (slots64 >= (1ull << 28)) return fail(c, PT_ERR_UNSUPPORTED, "frame too large: %llu slots (pixels of this rank x streams), limit 2^28", (unsigned long long)slots64); // kernels.hip at(): 32-bit byte offsets
    f.n_slots = (uint32_t)slots64;
    // every queue = kShards regions of shard_cap entries, one per shard. k_generate deals the 2^kShardGroupShift-slot groups out in
    // rotation: entry group t of shard s starts as slot group t * kShards + (s - t) mod kShards, so a shard owns ceil(groups / kShards)
    const uint32_t groups = (f.n_slots + (1u << kShardGroupShift) - 1u) >> kShardGroupShift, shard_cap = ((groups + kShards - 1) / kShards) << kShardGroupShift;
    f.shard_cap = shard_cap; f.q_entries = (size_t)kShards * shard_cap;
    f.samples_per_stream = (p->spp + f.streams - 1u) / f.streams;
    f.profile = (p->flags & PT_FLAG_PROFILE_KERNELS) != 0; f.count = (p->flags & PT_FLAG_COUNT_VISITS) != 0;
    f.bucket = (p->flags & PT_FLAG_BUCKET_SPECULAR) != 0; f.split = f.bucket || (p->flags & PT_FLAG_SPLIT_KERNELS) != 0;
    f.forced = (p->flags & PT_FLAG_EXTEND_POOL) ? (uint32_t)EXT_POOL : (p->flags & PT_FLAG_EXTEND_PACKED) ? (uint32_t)EXT_PACKED
               : (p->flags & PT_FLAG_EXTEND_SIMPLE) ? (uint32_t)EXT_SIMPLE : t.extend_kernel;
    // next-event estimation lives in the fused one-ray-per-lane kernel only. Its frames neither probe the extend kernel nor feed the
    // scene's choice (a forced kernel does neither), and they have no visit counters: a shadow ray's traversal stops at its tmax, which
    // §4.1's counters do not describe.
    f.nee = (p->flags & PT_FLAG_NEXT_EVENT) != 0;
    if (f.nee) {
        if (f.split || f.forced == (uint32_t)EXT_PACKED || f.forced == (uint32_t)EXT_POOL)
            return fail(c, PT_ERR_UNSUPPORTED, "PT_FLAG_NEXT_EVENT runs on the one-ray-per-lane kernel only: not with PT_FLAG_EXTEND_PACKED, "
                                               "PT_FLAG_EXTEND_POOL, PT_FLAG_SPLIT_KERNELS, PT_FLAG_BUCKET_SPECULAR or pt_tuning.extend_kernel 2 / 3");
        if (f.count) return fail(c, PT_ERR_UNSUPPORTED, "PT_FLAG_NEXT_EVENT does not count visits (PT_FLAG_COUNT_VISITS)");
        f.forced = EXT_SIMPLE;
    }
    // the fused one-ray-per-lane and lane-packing kernels build a slot's initial state in registers in their first launch; k_shade
    // (split pipelines) and the pooled kernel read it from memory
    f.full_state = f.split || f.forced == (uint32_t)EXT_POOL;
    f.mapped = t.readback == 0u; // queue sizes reach the host by the kernels' own stores (fold_traced) instead of a copy per launch
    // rays per wavefront of the lane-packing kernel: 256 once several sample streams keep the queues long, else 128 (measured)
    f.packed_chunk = t.packed_chunk >= 64u ? t.packed_chunk : (f.streams >= 4u ? 256u : 128u);
    // path vertices per launch of the one-ray-per-lane kernel: 3/4 max_depth - 2 (saturating), clamped to [4, 12]
    const uint32_t v34 = p->max_depth * 3u / 4u; f.default_bounces = std::min(12u, std::max(4u, v34 > 2u ? v34 - 2u : 0u));
    // NEE: `bounces` counts rays, and a vertex with a light sample takes two (shadow, then extension): twice the passes for about as many
    // vertices per launch
    if (f.nee) f.default_bounces *= 2u;
    // Iterations the host runs ahead of the queue sizes it reads back (pt_tuning.lag). The frame ends `lag` launches after its last path, on
    // grids sized `lag` iterations ago: short frames feel that (ms per 1080p frame with lag 4 / 3 / 2, tools/exp_lag.py: 1 spp 0.567 / 0.537 /
    // 0.529, 8 spp 2.79 / 2.73 / 2.70, glass 8 spp 1.57 / 1.52 / 1.48), long ones not (64 spp 17.73 / 17.68 / 17.73; a rank's 1/8 2.63 / 2.59 /
    // 2.61), and the lane-packing kernel's short tail launches want the host further ahead (soup 72.3 / 72.4 / 73.1). At least 2: the launch
    // after the last one that had paths clears that one's counter line. With the sizes stored by the kernels themselves (pt_tuning.readback =
    // 0) iteration j's line is written by launch j + 1, so the same run-ahead of the GPU takes one more iteration of lag than with a copy.
    f.lag = t.lag ? t.lag : (f.samples_per_stream <= 2u ? 2u : 3u) + (f.mapped ? 1u : 0u);
    // progressive accumulation (the reference re-renders every frame, App.cs:39-42; this is its converging analogue):
    // keep the stream partials of the previous call(s) and divide by the total number of samples at the end
    f.accumulate = (p->flags & PT_FLAG_ACCUMULATE) != 0;
    if (f.accumulate) {
        if (c->acc_spp == 0 || c->acc_w != p->width || c->acc_h != p->height || c->acc_rank != p->rank || c->acc_nranks != f.nranks ||
            c->acc_streams != f.streams || c->acc_seed != p->seed)
            return fail(c, PT_ERR_INVALID_ARGUMENT, "PT_FLAG_ACCUMULATE needs a previous frame with the same size, rank, nranks, streams and seed");
        if (c->acc_nee != f.nee)
            return fail(c, PT_ERR_INVALID_ARGUMENT, "PT_FLAG_ACCUMULATE: the sums so far were made %s PT_FLAG_NEXT_EVENT", c->acc_nee ? "with" : "without");
        if (p->sample_offset != c->acc_spp) return fail(c, PT_ERR_INVALID_ARGUMENT, "PT_FLAG_ACCUMULATE: sample_offset must be %llu (samples so far)", (unsigned long long)c->acc_spp);
    }
    f.total_spp = (f.accumulate ? c->acc_spp : 0u) + p->spp; c->acc_spp = 0; // acc_spp: invalid until this frame completes
    f.allocs_before = g_device_allocs;
    HIP_TRY(c, c->ray_o.ensure(f.n_slots)); HIP_TRY(c, c->ray_d.ensure(f.n_slots)); HIP_TRY(c, c->thr.ensure(f.n_slots));
    HIP_TRY(c, c->acc.ensure(f.n_slots)); HIP_TRY(c, c->tiles.ensure(f.pixel_slots)); HIP_TRY(c, c->sd.ensure(f.n_slots));
    HIP_TRY(c, c->q_ext0.ensure(f.q_entries)); HIP_TRY(c, c->q_ext1.ensure(f.q_entries));
    // hit records and the metal / dielectric buckets are k_shade's (no kernel indexes the miss and Lambert buckets)
    if (f.split) { HIP_TRY(c, c->hit.ensure(f.n_slots)); HIP_TRY(c, c->q_metal.ensure(f.q_entries)); HIP_TRY(c, c->q_dielectric.ensure(f.q_entries)); }
    if (!f.full_state) { HIP_TRY(c, c->q_init.ensure(f.q_entries)); HIP_TRY(c, c->cnt_init.ensure(kCntTotalWords)); }
    const uint32_t ovf = s->tree.stack_overflow();
    if (ovf) HIP_TRY(c, c->stack_ovf.ensure((size_t)ovf * f.q_entries));
    if (f.nee) {
        HIP_TRY(c, c->nee_ext.ensure(f.n_slots)); HIP_TRY(c, c->nee_rad.ensure(f.n_slots));
        f.nee_args = NeeArgs{ s->d_lights.p, s->d_cdf.p, s->d_pa.p, s->n_lights, c->nee_ext.p, c->nee_rad.p };
    }
    if (f.nranks == 1) { const pt_status st = ensure_frame(c, p->width, p->height); if (st != PT_OK) return st; }
    PathState &ps = f.ps;
    ps.ray_o = c->ray_o.p; ps.ray_d = c->ray_d.p; ps.thr = c->thr.p; ps.sd = c->sd.p; ps.acc = c->acc.p; ps.q_ext[0] = c->q_ext0.p; ps.q_ext[1] = c->q_ext1.p;
    if (f.split) { ps.hit = c->hit.p; ps.q_bucket[B_METAL] = c->q_metal.p; ps.q_bucket[B_DIELECTRIC] = c->q_dielectric.p; }
    ps.counters = c->counters.p; ps.stack_ovf = c->stack_ovf.p; ps.stack_ovf_entries = ovf; ps.n_slots = f.n_slots; ps.shard_cap = f.shard_cap;
    ps.shard_base = 0; ps.shard_count = kShards; ps.compact_below = t.compact_below; ps.finish_below = t.finish_below; ps.sparse_below = t.sparse_below;
    ps.repack_sticky = (f.samples_per_stream <= t.sticky_samples && t.compact_below > 0.f) ? 1u : 0u;
    ps.host_ring = f.mapped ? c->h_ring.d : nullptr; ps.ring_slots = kLag;
    // re-packing forced: buckets re-append (no fixed positions), or next to nothing regenerates (every launch leaves holes)
    f.compact = f.bucket || (ps.repack_sticky && f.samples_per_stream <= 2u);
    FrameParams &fp = f.fp;
    fp.width = p->width; fp.height = p->height; fp.spp = p->spp; fp.max_depth = p->max_depth; fp.rr_start = p->rr_start;
    fp.seed_hashed = host_pcg(p->seed); fp.sample_offset = p->sample_offset; fp.ray_eps = p->ray_eps;
    fp.rank = p->rank; fp.nranks = f.nranks; fp.tiles_x = lay.tiles_x; fp.n_tiles = lay.n_tiles; fp.streams = f.streams; fp.slots_per_stream = f.pixel_slots;
    div_magic(f.streams, fp.streams_magic, fp.streams_shift); div_magic(lay.tiles_x, fp.tiles_x_magic, fp.tiles_x_shift);
    fp.offset_mod = p->sample_offset % f.streams; fp.accumulate = f.accumulate ? 1u : 0u;
    return PT_OK;
}

// Start: the first extend queue and counter block, after ev_start. A full-state frame runs k_generate over every slot; a fused one copies the
// template of its geometry (pt_context::q_init: k_generate's output depends on which slots exist and on whether every stream has a sample).
static pt_status start_frame(pt_context *c, const pt_scene *s, const pt_render_params *p, const Frame &f)
{
    hipStream_t q = c->stream;
    if (f.full_state) {
        HIP_TRY(c, hipMemsetAsync(c->counters.p, 0, sizeof(uint32_t) * kCntTotalWords, q));
        HIP_TRY(c, hipEventRecord(c->ev_start, q));
        HIP_TRY(c, launch_generate(q, s->ds, f.ps, f.fp, 1u));
    } else {
        HIP_TRY(c, hipEventRecord(c->ev_start, q));
        pt_context::InitKey key; std::memset(&key, 0, sizeof key); // (compared bytewise: padding included)
        key.w = p->width; key.h = p->height; key.rank = p->rank; key.nranks = f.nranks; key.streams = f.streams; key.first_spp = std::min(p->spp, f.streams);
        key.offset = f.fp.offset_mod; key.n_slots = f.n_slots; key.shard_cap = f.shard_cap; key.q = c->q_init.p; key.acc = c->acc.p;
        if (!c->init_valid || !(key == c->init_key)) {
            c->init_valid = false; HIP_TRY(c, hipMemsetAsync(c->cnt_init.p, 0, sizeof(uint32_t) * kCntTotalWords, q));
            PathState pt = f.ps; pt.counters = c->cnt_init.p; pt.q_ext[0] = c->q_init.p;
            // whole streams without a sample (spp < streams): the first queue holds the live slots only, and the first launch is sized by it
            const bool dense = key.first_spp < f.streams;
            HIP_TRY(c, launch_generate(q, s->ds, pt, f.fp, dense ? 2u : 0u)); // also zeroes every slot's sum unless the frame accumulates
            c->init_bound = f.shard_cap;
            if (dense) {
                HIP_TRY(c, hipMemcpyAsync(c->h_counts.p + kFinalOffset, c->cnt_init.p, sizeof(uint32_t) * kShards * kCounterStride, hipMemcpyDeviceToHost, q));
                HIP_TRY(c, hipStreamSynchronize(q));
                c->init_bound = 0;
                for (uint32_t sh = 0; sh < kShards; ++sh) c->init_bound = std::max(c->init_bound, c->h_counts.p[kFinalOffset + cnt_ext_index(0, sh)]);
            }
            c->init_key = key; c->init_valid = true;
        }
        HIP_TRY(c, hipMemcpyAsync(c->counters.p, c->cnt_init.p, sizeof(uint32_t) * kCntTotalWords, hipMemcpyDeviceToDevice, q));
    }
    // the template invariant (pt_context::q_init): this frame writes the streams a dense template leaves out
    if ((f.accumulate || f.full_state) && c->init_key.first_spp < c->init_key.streams) c->init_valid = false;
    return PT_OK;
}

// Loops. Shards never exchange slots, so the 64 shards are split into `n_loops` independent loops, each on its own HIP stream: the tail of one
// group's launch (its last wavefronts draining) is filled by the other's launch (pt_tuning.loops has the measurements). Inside a loop a shard's
// queue can only shrink (slots die, none are born), so the queue sizes read back `lag` iterations ago are valid launch bounds: the host never
// stalls the GPU to size a grid. Queues are carried over IN PLACE from one iteration to the next: a lane writes its own queue position, dead
// paths leave holes, and lane <-> slot stays the generation order, so the slot-indexed state keeps its coalescing and no returning atomic is
// needed. A shard re-packs its survivors (ballot + atomic append) in the iteration in which its alive/length ratio is below `compact_below`,
// and runs its last `finish_below` paths to their end in one launch; both are decided by the kernels from the shard's counters, the host only
// sizes grids and notices the end.
static pt_status run_loops(pt_context *c, const pt_scene *s, const pt_render_params *p, Frame &f, ExtendFrame &x)
{
    hipStream_t q = c->stream; const uint32_t n_loops = f.n_loops, per_group = kShards / n_loops;
    struct Loop { hipStream_t stream; uint32_t base, bound, iters; bool done; } loops[kMaxGroups];
    HIP_TRY(c, hipEventRecord(c->ev_fork, q));
    for (uint32_t g = 0; g < n_loops; ++g) {
        loops[g] = Loop{ n_loops == 1 ? q : c->group_stream[g], g * per_group, f.full_state ? f.shard_cap : c->init_bound, 0u, false }; // no shard's queue can outgrow its first one
        if (loops[g].stream != q) HIP_TRY(c, hipStreamWaitEvent(loops[g].stream, c->ev_fork, 0));
    }
    const uint64_t max_iters = (uint64_t)p->spp * p->max_depth * (f.nee ? 2u : 1u) + kLag + 2; // NEE: up to two rays per vertex
    const bool trace = f.profile && getenv("PTRT_TRACE") != nullptr; // developer aid: per-iteration table on stderr
    // One kernel per iteration by default: every extend kernel (one ray per lane, lane-packing, pooled) shades its own hits (mode 0:
    // Lambert-only scene, lean code; 2: all kinds). PT_FLAG_SPLIT_KERNELS / _BUCKET_SPECULAR run k_shade as a second kernel.
    const int shade_mode = s->has_specular ? 2 : 0;
    for (uint32_t live = n_loops; live > 0;) {
        for (uint32_t g = 0; g < n_loops; ++g) {
            Loop &L = loops[g];
            if (L.done) continue;
            if (L.iters >= max_iters) return fail(c, PT_ERR_INTERNAL, "wavefront loop did not drain after %u iterations", L.iters);
            const uint32_t it = L.iters; PathState pg = f.ps; pg.shard_base = L.base; pg.shard_count = per_group;
            if (it == 0u && !f.full_state) pg.q_ext[0] = c->q_init.p; // the frame's first queue is the template: read, never written
            if (x.kernel == 0u) pg.finish_below = 0u; // probing: no finish mode
            hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
            if (f.profile) {
                e0 = pool_event(c, f.n_events++); e1 = pool_event(c, f.n_events++); e2 = pool_event(c, f.n_events++);
                if (!e0 || !e1 || !e2) return fail(c, PT_ERR_HIP, "hipEventCreate failed"); // (the text this failure has always had)
                HIP_TRY(c, hipEventRecord(e0, L.stream));
            }
            const bool probing = x.probing(g, it); const int kernel = x.launch_kernel(g, it, f.split);
            if (probing) HIP_TRY(c, hipEventRecord(c->ev_probe[(it - 2u) * 2u], L.stream));
            HIP_TRY(c, launch_extend(L.stream, s->ds, pg, f.fp, it, L.bound, f.count, kernel, f.packed_chunk, f.split ? -1 : shade_mode, f.compact,
                                     c->tuning.bounces ? c->tuning.bounces : x.bounces(g, it, kernel, f.default_bounces), f.nee ? &f.nee_args : nullptr));
            if (f.profile) HIP_TRY(c, hipEventRecord(e1, L.stream));
            if (f.bucket) {
                HIP_TRY(c, launch_shade(L.stream, s->ds, pg, f.fp, it, L.bound, 0, true));
                HIP_TRY(c, launch_shade(L.stream, s->ds, pg, f.fp, it, L.bound, 1, true)); // metal + dielectric buckets
            } else if (f.split) HIP_TRY(c, launch_shade(L.stream, s->ds, pg, f.fp, it, L.bound, shade_mode, f.compact));
            if (probing) HIP_TRY(c, hipEventRecord(c->ev_probe[(it - 2u) * 2u + 1u], L.stream)); // the whole iteration, either way
            if (f.profile) HIP_TRY(c, hipEventRecord(e2, L.stream));
            const uint32_t ring = L.iters % kLag;
            if (!f.mapped) {
                uint32_t *h_ring = c->h_counts.p + ((size_t)g * kLag + ring) * kRingWords;
                HIP_TRY(c, hipMemcpyAsync(h_ring, c->counters.p + cnt_ext_index((it + 1u) % 3u, L.base), sizeof(uint32_t) * per_group * kCounterStride,
                                          hipMemcpyDeviceToHost, L.stream));
            }
            HIP_TRY(c, hipEventRecord(c->ev_lag[g][ring], L.stream));
            f.iters = std::max(f.iters, ++L.iters);
            if (L.iters < f.lag) continue;
            const uint32_t old_iter = L.iters - f.lag; // iteration old_iter traced `traced` rays and left `total` paths alive: its survivors bound every later queue
            // mapped: launch old_iter + 1 stored old_iter's lines (fold_traced); it is at most the launch just enqueued since lag >= 2
            HIP_TRY(c, hipEventSynchronize(c->ev_lag[g][(f.mapped ? old_iter + 1u : old_iter) % kLag]));
            const volatile uint32_t *h_old = f.mapped ? (const volatile uint32_t *)(c->h_ring.p + (size_t)(old_iter % kLag) * kShards + L.base)
                                                      : c->h_counts.p + ((size_t)g * kLag + old_iter % kLag) * kRingWords;
            // a shard's line: word 0 = queue length (holes included), word 1 = alive entries, words 2-3 = rays the iteration traced
            const uint32_t line = f.mapped ? 4u : kCounterStride;
            uint32_t mx = 0; uint64_t total = 0, traced = 0;
            for (uint32_t sh = 0; sh < per_group; ++sh) {
                mx = std::max(mx, (uint32_t)h_old[sh * line]);
                total += h_old[sh * line + 1];
                traced += (uint64_t)h_old[sh * line + 2] | ((uint64_t)h_old[sh * line + 3] << 32);
            }
            L.bound = mx;
            if (trace) {
                f.trace_alive.resize(std::max<size_t>(f.trace_alive.size(), old_iter + 1), 0); f.trace_rays.resize(f.trace_alive.size(), 0);
                f.trace_alive[old_iter] += total; f.trace_rays[old_iter] += traced;
            }
            f.slot_launches += total; // = paths alive at the start of iteration old_iter + 1 (those read after the loop ended are all 0)
            if (total == 0) { L.done = true; --live; }
            HIP_TRY(c, x.observe(g, old_iter, traced, f.n_slots / n_loops, c->ev_probe));
        }
    }
    for (uint32_t g = 0; g < n_loops; ++g) // join: the main stream continues after every group's last kernel
        if (loops[g].stream != q) { HIP_TRY(c, hipEventRecord(c->ev_join[g], loops[g].stream)); HIP_TRY(c, hipStreamWaitEvent(q, c->ev_join[g], 0)); }
    return PT_OK;
}

// Finish: reduce the streams and assemble, read every counter back, check that the frame ended clean, fill pt_stats
static pt_status finish_frame(pt_context *c, const pt_render_params *p, const Frame &f, ExtendFrame &x, pt_stats *stats)
{
    hipStream_t q = c->stream; const FrameParams &fp = f.fp;
    HIP_TRY(c, launch_reduce_streams(q, c->acc.p, c->tiles.p, f.pixel_slots, f.streams)); // tiles = the pixel sums = the gather payload
    if (f.nranks == 1)
        HIP_TRY(c, launch_assemble(q, c->tiles.p, 1, f.pixel_slots, p->width, p->height, fp.tiles_x, fp.n_tiles, 1.0f / (float)f.total_spp, c->fb.p, c->fb8.p));
    HIP_TRY(c, hipEventRecord(c->ev_stop, q));
    HIP_TRY(c, hipMemcpyAsync(c->h_counts.p + kFinalOffset, c->counters.p, sizeof(uint32_t) * kCntTotalWords, hipMemcpyDeviceToHost, q));
    HIP_TRY(c, hipStreamSynchronize(q));
    pt_stats out{}; const uint32_t *hc = c->h_counts.p + kFinalOffset;
    if (hc[kCntError]) return fail(c, PT_ERR_INTERNAL, "device error flag 0x%x (1 = traversal stack overflow, 2 = step limit)", hc[kCntError]);
    auto u64_at = [&](uint32_t w) { return (uint64_t)hc[w] | ((uint64_t)hc[w + 1] << 32); };
    for (uint32_t sh = 0; sh < kShards; ++sh) {
        if (hc[cnt_alive_index(0, sh)] || hc[cnt_alive_index(1, sh)] || hc[cnt_alive_index(2, sh)]) return fail(c, PT_ERR_INTERNAL, "extend queue of shard %u not empty at frame end", sh);
        out.rays += u64_at(cnt_rays_index(sh));
    }
    float ms = 0.f; HIP_TRY(c, hipEventElapsedTime(&ms, c->ev_start, c->ev_stop)); out.gpu_ms = ms;
    out.node_visits = u64_at(kCntNodes); out.tri_tests = u64_at(kCntTris); out.sphere_tests = u64_at(kCntSph);
    // PT_FLAG_COUNT_VISITS + one-ray-per-lane kernel: wave-level node-loop iterations (bits 0-39) and, from bit 40 up, how many
    // of them came after the wave's first leaf phase of the ray (diagnostic for tools/exp_util.py)
    out.reserved[3] = (u64_at(kCntWaveNodeIters) & 0xFFFFFFFFFFull) | (u64_at(kCntWaveNodeIters + 2) << 40);
    if (f.count && getenv("PTRT_TRACE")) { // developer aid: where the node loop's lane-slots go (one-ray-per-lane kernel)
        const double slots = 64.0 * (double)u64_at(kCntWaveNodeIters), v = (double)out.node_visits, lf = (double)u64_at(kCntIdleLeaf), dn = (double)u64_at(kCntIdleDone);
        if (slots > 0) fprintf(stderr, "ptrt: node-loop lane-slots %.3g: visiting %.1f %%, waiting at a leaf %.1f %%, ray finished %.1f %%, no ray %.1f %%\n", slots,
                               100 * v / slots, 100 * lf / slots, 100 * dn / slots, 100 * (slots - v - lf - dn) / slots);
    }
    out.iterations = f.iters; out.extend_launches = f.iters;
    x.frame_done(out.rays, out.gpu_ms, g_device_allocs != f.allocs_before);
    out.reserved[0] = x.kernel ? x.kernel : (uint32_t)EXT_SIMPLE; // extend kernel in use at frame end (ExtendKernel)
    out.reserved[1] = hc[kCntCompactions]; // (shard, iteration) pairs that re-packed their queue (the others carried it over in place)
    uint64_t px = 0; // paths = owned in-image pixels x spp
    for (uint32_t t = p->rank; t < fp.n_tiles; t += f.nranks) {
        const uint32_t tx = t % fp.tiles_x, ty = t / fp.tiles_x;
        px += (uint64_t)std::min(kTile, p->width - tx * kTile) * std::min(kTile, p->height - ty * kTile);
    }
    out.paths = px * p->spp;
    // path states read + written by the wavefront loop = sum over launches of the paths alive at launch start
    // (iteration 0 starts every (pixel, stream) pair that has a sample)
    out.reserved[2] = f.slot_launches + px * std::min(f.streams, p->spp);
    if (f.profile) {
        const bool trace = getenv("PTRT_TRACE") != nullptr;
        for (size_t i = 0; i + 2 < f.n_events; i += 3) { // three events per iteration: before extend, between, after shade
            float a = 0.f, b = 0.f; HIP_TRY(c, hipEventElapsedTime(&a, c->ev_pool[i], c->ev_pool[i + 1]));
            HIP_TRY(c, hipEventElapsedTime(&b, c->ev_pool[i + 1], c->ev_pool[i + 2]));
            out.extend_ms += a; out.shade_ms += b;
            if (trace) fprintf(stderr, "ptrt: iteration %3zu  rays %10llu  alive after %10llu  extend %8.3f ms  shade %8.3f ms\n", i / 3,
                               (unsigned long long)(i / 3 < f.trace_rays.size() ? f.trace_rays[i / 3] : 0),
                               (unsigned long long)(i / 3 < f.trace_alive.size() ? f.trace_alive[i / 3] : 0), a, b);
        }
        out.other_ms = out.gpu_ms - out.extend_ms - out.shade_ms;
    }
    c->n_slots = f.pixel_slots; c->acc_w = p->width; c->acc_h = p->height; c->acc_rank = p->rank; c->acc_nranks = f.nranks; c->acc_streams = f.streams; c->acc_seed = p->seed;
    c->acc_spp = f.total_spp; c->acc_nee = f.nee; c->fb_valid = (f.nranks == 1);
    if (stats) *stats = out;
    return PT_OK;
}

static pt_status render_frame(pt_context *c, const pt_scene *s, const pt_render_params *p, pt_stats *stats)
{
    if (!c || !p) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_render: NULL argument");
    pt_tile_layout lay; pt_status st = layout_of(p, &lay);
    if (st != PT_OK) return fail(c, st, "pt_render: bad width/height/rank/nranks/tile_size");
    HIP_TRY(c, hipSetDevice(c->device));
    c->fb_valid = false; c->fb_reference = false;
    c->dn_guides = c->dn_image = false; // the denoised results belong to the frame this call replaces
    if (p->mode == PT_REFERENCE_SPHERE) { // Renderer.ComputeFrame: one dispatch, then the host blocks on the fence (Renderer.cs:1020,1036,972)
        if ((st = ensure_frame(c, p->width, p->height)) != PT_OK) return st;
        HIP_TRY(c, hipEventRecord(c->ev_start, c->stream));
        HIP_TRY(c, launch_reference_sphere(c->stream, p->width, p->height, c->fb.p, c->fb8.p));
        HIP_TRY(c, hipEventRecord(c->ev_stop, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        float ms = 0.f; HIP_TRY(c, hipEventElapsedTime(&ms, c->ev_start, c->ev_stop));
        pt_stats out{};
        out.gpu_ms = ms; out.other_ms = ms; out.rays = out.paths = (uint64_t)p->width * p->height; out.iterations = 1;
        c->fb_valid = true; c->fb_reference = true; if (stats) *stats = out;
        return PT_OK;
    }
    if (p->mode != PT_PATH_TRACE) return fail(c, PT_ERR_INVALID_ARGUMENT, "unknown mode %u", p->mode);
    Frame f{};
    if ((st = plan_frame(c, s, p, lay, f)) != PT_OK) return st;
    ExtendFrame x(s->cache.ext, f.forced, f.count || f.profile);
    f.n_loops = (f.profile || f.count || x.kernel == 0u) ? 1u : c->tuning.loops ? c->tuning.loops : 2u; // timed kernels run alone
    if ((st = start_frame(c, s, p, f)) != PT_OK || (st = run_loops(c, s, p, f, x)) != PT_OK) return st;
    return finish_frame(c, p, f, x, stats);
}

pt_status pt_render(pt_context *c, const pt_scene *s, const pt_render_params *p, pt_stats *stats)
{
    const pt_status st = drained_on_failure(c, [&] { return render_frame(c, s, p, stats); });
    if (st != PT_OK && c) { c->acc_spp = 0; c->fb_valid = false; } // nothing of this frame survives the call
    return st;
}

// ------------------------------------------------------------------------------------------------ ray queries (docs/SPEC.md §4.2)

// The plumbing of a query (pt_trace_rays, pt_denoise's guide pass): the context's own counter block and overflow area, never pt_render's
// (the frame-start template, the partial sums, the queues and their counters stay untouched). trace_setup sizes the overflow area for
// launches of up to n_rays rays and zeroes the counter words the kernels use; trace_launch enqueues the launches (k_trace indexes with 32
// bits); trace_readback copies those words back (error flag first, then the visit counters) for the caller's synchronise.
constexpr uint64_t kTraceChunk = 1ull << 31;                   // rays per launch
constexpr uint32_t kTraceWords = kCntTotalWords - kCntGlobals; // the counter words of a query
static pt_status trace_setup(pt_context *c, const pt_scene *s, uint64_t n_rays, PathState &ps)
{
    const uint32_t blocks = trace_blocks((uint32_t)std::min<uint64_t>(n_rays, kTraceChunk)), lanes = blocks * kExtBlock;
    ps = PathState{};
    ps.shard_cap = (lanes + kShards - 1u) / kShards; // one overflow column per lane of the grid, reused by its every ray
    ps.stack_ovf_entries = s->tree.stack_overflow();
    if (ps.stack_ovf_entries) HIP_TRY(c, c->trace_ovf.ensure((size_t)ps.stack_ovf_entries * kShards * ps.shard_cap));
    ps.stack_ovf = c->trace_ovf.p;
    HIP_TRY(c, c->trace_cnt.ensure(kCntTotalWords)); // the kernels use the global words only: error flag and visit counters
    ps.counters = c->trace_cnt.p;
    HIP_TRY(c, hipMemsetAsync(c->trace_cnt.p + kCntGlobals, 0, sizeof(uint32_t) * kTraceWords, c->stream));
    return PT_OK;
}
static pt_status trace_launch(pt_context *c, const pt_scene *s, const PathState &ps, const float4 *rays, float4 *hits, uint64_t n_rays,
                              bool occlusion, bool count)
{
    for (uint64_t first = 0; first < n_rays; first += kTraceChunk)
        HIP_TRY(c, launch_trace(c->stream, s->ds, ps, rays + 2u * first, hits + first, (uint32_t)std::min(kTraceChunk, n_rays - first), occlusion, count));
    return PT_OK;
}
static pt_status trace_readback(pt_context *c, uint32_t (&hc)[kTraceWords])
{
    HIP_TRY(c, hipMemcpyAsync(hc, c->trace_cnt.p + kCntGlobals, sizeof hc, hipMemcpyDeviceToHost, c->stream));
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
    if ((st = trace_setup(c, s, n_rays, ps)) != PT_OK) return st;
    const float4 *d_rays = (const float4 *)rays;
    float4 *d_hits = (float4 *)hits;
    if (host) { // staged through the context's own buffers
        HIP_TRY(c, c->trace_rays.ensure((size_t)n_rays * 2u)); HIP_TRY(c, c->trace_hits.ensure((size_t)n_rays));
        HIP_TRY(c, hipMemcpyAsync(c->trace_rays.p, rays, n_rays * 32u, hipMemcpyHostToDevice, q));
        d_rays = c->trace_rays.p; d_hits = c->trace_hits.p;
    }
    HIP_TRY(c, hipEventRecord(c->ev_trace[0], q));
    if ((st = trace_launch(c, s, ps, d_rays, d_hits, n_rays, occlusion, count)) != PT_OK) return st;
    HIP_TRY(c, hipEventRecord(c->ev_trace[1], q));
    if (host) HIP_TRY(c, hipMemcpyAsync(hits, d_hits, n_rays * 16u, hipMemcpyDeviceToHost, q));
    uint32_t hc[kTraceWords];
    if ((st = trace_readback(c, hc)) != PT_OK) return st;
    HIP_TRY(c, hipStreamSynchronize(q));
    if (hc[kCntError - kCntGlobals])
        return fail(c, PT_ERR_INTERNAL, "pt_trace_rays: device error flag 0x%x (1 = traversal stack overflow, 2 = step limit)", hc[kCntError - kCntGlobals]);
    auto u64_at = [&](uint32_t w) { return (uint64_t)hc[w - kCntGlobals] | ((uint64_t)hc[w - kCntGlobals + 1] << 32); };
    float ms = 0.f; HIP_TRY(c, hipEventElapsedTime(&ms, c->ev_trace[0], c->ev_trace[1])); out.gpu_ms = ms;
    if (count) { out.node_visits = u64_at(kCntNodes); out.tri_tests = u64_at(kCntTris); out.sphere_tests = u64_at(kCntSph); }
    if (stats) *stats = out;
    return PT_OK;
}

pt_status pt_trace_rays(pt_context *c, const pt_scene *s, const void *rays, void *hits, uint64_t n_rays, uint32_t flags, pt_stats *stats)
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
    if (c->fb_valid && c->fb_reference) return fail(c, PT_ERR_UNSUPPORTED, "pt_denoise: the framebuffer holds a PT_REFERENCE_SPHERE frame");
    if (!c->fb_valid) return fail(c, PT_ERR_NOT_COMMITTED, "pt_denoise: no assembled frame (render with nranks == 1 or assemble the tiles first)");
    const bool guides_only = (dp->flags & PT_DENOISE_GUIDES_ONLY) != 0;
    const uint32_t passes = guides_only ? 0u : dp->iterations ? dp->iterations : kDenoiseIterations;
    const float sc = sigma[0] != 0.0f ? sigma[0] : kSigmaColor, sn = sigma[1] != 0.0f ? sigma[1] : kSigmaNormal;
    const float sz = sigma[2] != 0.0f ? sigma[2] : kSigmaDepth, sa = sigma[3] != 0.0f ? sigma[3] : kSigmaAlbedo;

    const uint32_t w = c->fb_w, h = c->fb_h;
    const size_t n = (size_t)w * h;
    HIP_TRY(c, hipSetDevice(c->device));
    for (auto &e : c->ev_denoise) HIP_TRY(c, e.create());
    c->dn_guides = c->dn_image = false; // from here on the buffers are rewritten
    HIP_TRY(c, c->dn_work.ensure(2 * n)); HIP_TRY(c, c->dn_hits.ensure(n));
    HIP_TRY(c, c->dn_g0.ensure(n)); HIP_TRY(c, c->dn_g1.ensure(n));
    if (passes) HIP_TRY(c, c->dn_out.ensure(n));
    const uint32_t nt = s->ds.n_tris;
    if (!s->cache.blob_of_ready) HIP_TRY(c, s->cache.d_blob_of.ensure(std::max<size_t>(nt, 1)));
    pt_status st;
    PathState ps;
    if ((st = trace_setup(c, s, n, ps)) != PT_OK) return st;
    hipStream_t q = c->stream;
    HIP_TRY(c, hipEventRecord(c->ev_denoise[0], q));
    if (!s->cache.blob_of_ready) { // (zeroed first: every entry is a valid blob index even if an id were missing)
        HIP_TRY(c, hipMemsetAsync(s->cache.d_blob_of.p, 0, std::max<size_t>(nt, 1) * sizeof(uint32_t), q));
        HIP_TRY(c, launch_guide_index(q, s->ds.tris, nt, s->cache.d_blob_of.p));
    }
    float4 *rays = c->dn_work.p;
    HIP_TRY(c, launch_guide_rays(q, s->cam, w, h, rays));
    if ((st = trace_launch(c, s, ps, rays, c->dn_hits.p, n, false, false)) != PT_OK) return st;
    HIP_TRY(c, launch_guide_resolve(q, s->ds, s->cache.d_blob_of.p, rays, c->dn_hits.p, (uint32_t)n, c->dn_g0.p, c->dn_g1.p));
    HIP_TRY(c, hipEventRecord(c->ev_denoise[1], q));
    // pass i reads the framebuffer (i = 0) or pass i-1's image; the last pass writes dn_out, the others alternate between the two halves
    // of dn_work (the rays are dead by then)
    AtrousParams ap{};
    ap.width = w; ap.height = h; ap.edge_stops = (dp->flags & PT_DENOISE_NO_EDGE_STOPS) == 0;
    ap.inv_sn = atrous_scale(1.0f / sn); ap.sigma_z = sz; ap.ia = atrous_scale(1.0f / (sa * sa));
    const float ic = 1.0f / (sc * sc);
    const float4 *src = c->fb.p;
    for (uint32_t i = 0; i < passes; ++i) {
        float4 *dst = i + 1 == passes ? c->dn_out.p : c->dn_work.p + (i & 1u) * n;
        ap.pass = i; ap.ic_i = atrous_scale(ic * (float)(1u << (2u * i)));
        HIP_TRY(c, launch_atrous(q, ap, src, c->dn_g0.p, c->dn_g1.p, dst));
        src = dst;
    }
    HIP_TRY(c, hipEventRecord(c->ev_denoise[2], q));
    uint32_t hc[kTraceWords];
    if ((st = trace_readback(c, hc)) != PT_OK) return st;
    HIP_TRY(c, hipStreamSynchronize(q));
    if (hc[kCntError - kCntGlobals])
        return fail(c, PT_ERR_INTERNAL, "pt_denoise: device error flag 0x%x in the guide pass (1 = traversal stack overflow, 2 = step limit)", hc[kCntError - kCntGlobals]);
    s->cache.blob_of_ready = true;
    float ms_guides = 0.f, ms_filter = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms_guides, c->ev_denoise[0], c->ev_denoise[1]));
    HIP_TRY(c, hipEventElapsedTime(&ms_filter, c->ev_denoise[1], c->ev_denoise[2]));
    pt_stats out{};
    out.rays = n; out.iterations = passes;
    out.extend_ms = ms_guides; out.other_ms = ms_filter; out.gpu_ms = (double)ms_guides + ms_filter;
    c->dn_w = w; c->dn_h = h; c->dn_guides = true; c->dn_image = passes > 0;
    if (stats) *stats = out;
    return PT_OK;
}

pt_status pt_denoise(pt_context *c, const pt_scene *s, const pt_denoise_params *dp, pt_stats *stats)
{
    return drained_on_failure(c, [&] { return denoise(c, s, dp, stats); });
}

pt_status pt_denoised_read(pt_context *c, float *rgba, uint64_t n_floats)
{
    if (!c || !rgba) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_denoised_read: NULL argument");
    if (!c->dn_image) return fail(c, PT_ERR_NOT_COMMITTED, "pt_denoised_read: no denoised image (pt_denoise after the last pt_render, without PT_DENOISE_GUIDES_ONLY)");
    const uint64_t need = (uint64_t)c->dn_w * c->dn_h * 4;
    if (n_floats < need) return fail(c, PT_ERR_INVALID_ARGUMENT, "buffer too small: need %llu floats", (unsigned long long)need);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(rgba, c->dn_out.p, need * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PT_OK;
}

pt_status pt_denoised_device_ptr(pt_context *c, void **dptr, uint64_t *n_floats)
{
    if (!c || !dptr) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_denoised_device_ptr: NULL argument");
    if (!c->dn_image) return fail(c, PT_ERR_NOT_COMMITTED, "pt_denoised_device_ptr: no denoised image");
    *dptr = c->dn_out.p;
    if (n_floats) *n_floats = (uint64_t)c->dn_w * c->dn_h * 4;
    return PT_OK;
}

pt_status pt_guides_read(pt_context *c, float *g8, uint64_t n_floats)
{
    if (!c || !g8) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_guides_read: NULL argument");
    if (!c->dn_guides) return fail(c, PT_ERR_NOT_COMMITTED, "pt_guides_read: no guides (pt_denoise after the last pt_render)");
    const size_t n = (size_t)c->dn_w * c->dn_h;
    if (n_floats < (uint64_t)n * 8) return fail(c, PT_ERR_INVALID_ARGUMENT, "buffer too small: need %llu floats", (unsigned long long)n * 8);
    HIP_TRY(c, hipSetDevice(c->device));
    std::vector<float4> planes(2 * n); // the device keeps g0 and g1 as separate planes (one coalesced row each for the filter)
    HIP_TRY(c, hipMemcpyAsync(planes.data(), c->dn_g0.p, n * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(planes.data() + n, c->dn_g1.p, n * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < n; ++i) {
        std::memcpy(g8 + 8 * i, &planes[i], sizeof(float4));
        std::memcpy(g8 + 8 * i + 4, &planes[n + i], sizeof(float4));
    }
    return PT_OK;
}

pt_status pt_framebuffer_read(pt_context *c, float *rgba, uint64_t n_floats)
{
    if (!c || !rgba) return fail(c, PT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!c->fb_valid) return fail(c, PT_ERR_NOT_COMMITTED, "no assembled frame (render with nranks == 1 or call pt_assemble_tiles)");
    const uint64_t need = (uint64_t)c->fb_w * c->fb_h * 4;
    if (n_floats < need) return fail(c, PT_ERR_INVALID_ARGUMENT, "buffer too small: need %llu floats", (unsigned long long)need);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(rgba, c->fb.p, need * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PT_OK;
}

pt_status pt_framebuffer_read_rgba8(pt_context *c, uint8_t *rgba8, uint64_t n_bytes)
{
    if (!c || !rgba8) return fail(c, PT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!c->fb_valid) return fail(c, PT_ERR_NOT_COMMITTED, "no assembled frame");
    const uint64_t need = (uint64_t)c->fb_w * c->fb_h * 4;
    if (n_bytes < need) return fail(c, PT_ERR_INVALID_ARGUMENT, "buffer too small: need %llu bytes", (unsigned long long)need);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(rgba8, c->fb8.p, need, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PT_OK;
}

pt_status pt_framebuffer_read_srgb8(pt_context *c, uint8_t *rgba8, uint64_t n_bytes)
{
    // display transform of the reference (SwapChain.cs:157-158 B8G8R8A8Srgb target, nearest-sampled UNORM8 source): a function of
    // the 8-bit value, so it is a 256-entry table over the UNORM8 read-back; alpha is linear in sRGB formats
    pt_status st = pt_framebuffer_read_rgba8(c, rgba8, n_bytes);
    if (st != PT_OK) return st;
    uint8_t lut[256];
    for (int q = 0; q < 256; ++q) {
        const double l = q / 255.0, e = l <= 0.0031308 ? 12.92 * l : 1.055 * std::pow(l, 1.0 / 2.4) - 0.055;
        lut[q] = (uint8_t)std::floor(255.0 * e + 0.5);
    }
    const uint64_t n = (uint64_t)c->fb_w * c->fb_h * 4;
    for (uint64_t i = 0; i < n; ++i) if ((i & 3u) != 3u) rgba8[i] = lut[rgba8[i]];
    return PT_OK;
}

pt_status pt_framebuffer_device_ptr(pt_context *c, void **dptr, uint64_t *n_floats)
{
    if (!c || !dptr) return fail(c, PT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!c->fb_valid) return fail(c, PT_ERR_NOT_COMMITTED, "no assembled frame");
    *dptr = c->fb.p;
    if (n_floats) *n_floats = (uint64_t)c->fb_w * c->fb_h * 4;
    return PT_OK;
}

pt_status pt_tiles_device_ptr(pt_context *c, void **dptr, uint64_t *n_floats)
{
    if (!c || !dptr) return fail(c, PT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!c->n_slots) return fail(c, PT_ERR_NOT_COMMITTED, "no path-traced frame yet");
    *dptr = c->tiles.p;
    if (n_floats) *n_floats = (uint64_t)c->n_slots * 4;
    return PT_OK;
}

pt_status pt_assemble_tiles(pt_context *c, const pt_render_params *p, const void *gathered, uint64_t n_floats)
{
    if (!c || !p || !gathered) return fail(c, PT_ERR_INVALID_ARGUMENT, "NULL argument");
    pt_tile_layout lay;
    pt_status st = layout_of(p, &lay);
    if (st != PT_OK) return fail(c, st, "pt_assemble_tiles: bad params");
    if (p->spp == 0) return fail(c, PT_ERR_INVALID_ARGUMENT, "spp == 0");
    const uint32_t nranks = p->nranks ? p->nranks : 1u;
    const uint64_t per_rank = (uint64_t)lay.tiles_per_rank * kTilePixels;
    if (n_floats < per_rank * nranks * 4) return fail(c, PT_ERR_INVALID_ARGUMENT, "gathered buffer too small: need %llu floats", (unsigned long long)(per_rank * nranks * 4));
    HIP_TRY(c, hipSetDevice(c->device));
    c->fb_valid = false; c->fb_reference = false; c->dn_guides = c->dn_image = false;
    if ((st = ensure_frame(c, p->width, p->height)) != PT_OK) return st;
    HIP_TRY(c, launch_assemble(c->stream, (const float4 *)gathered, nranks, (uint32_t)per_rank, p->width, p->height, lay.tiles_x, lay.n_tiles,
                               1.0f / (float)(((p->flags & PT_FLAG_ACCUMULATE) ? (uint64_t)p->sample_offset : 0u) + p->spp), c->fb.p, c->fb8.p));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->fb_valid = true;
    return PT_OK;
}

} // extern "C"
