// frame.cpp — pt_render: the extend-kernel probe and the wavefront frame loop (plan, start, loops, finish) over the owners of context.h.
// Stands where Renderer.ComputeFrame + the compute-fence wait stand in the reference (RayTracing/Graphics/Renderer.cs:1006-1040, 970-972).
#include "scene.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace ptrt;

namespace {

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
// Which kernel one launch runs, given this frame's choice, is the pipeline's to say (pipeline.h Pipeline::kernel_for).
uint32_t faster(double rate_simple, double rate_packed) { return rate_packed > 1.10 * rate_simple ? EXT_PACKED : EXT_SIMPLE; }
struct ExtendFrame {            // the choice during one frame
    ExtendChoice &mem;
    bool undecided;             // nothing forces a kernel and the scene has not picked one: this frame measures (whole, on frame_kernel)
    uint32_t frame_kernel, kernel; // kernel: 0 = probing inside this frame, else the ExtendKernel every iteration uses
    bool mixed = false;         // this frame ran probe iterations on both kernels: its overall rate says nothing about either
    uint64_t probe_n[2] = { 0, 0 }; // rays traced by probe iterations 2 and 3
    ExtendFrame(ExtendChoice &m, const Pipeline &p) : mem(m),
        undecided(p.forced == 0u && m.kernel == 0u && !p.instrumented()),
        frame_kernel((undecided && m.rate_simple > 0.0 && m.rate_packed == 0.0) ? EXT_PACKED : EXT_SIMPLE), // first the default, then the other
        kernel(p.forced ? p.forced : m.kernel ? m.kernel : (undecided && frame_kernel == EXT_SIMPLE) ? 0u : frame_kernel) {}
    bool probing(uint32_t g, uint32_t it) const { return g == 0u && kernel == 0u && (it == 2u || it == 3u); }
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

hipEvent_t pool_event(pt_context *c, size_t i)
{
    while (c->ev_pool.size() <= i) {
        Event e;
        if (e.create() != hipSuccess) return nullptr;
        c->ev_pool.push_back(std::move(e));
    }
    return c->ev_pool[i];
}

// The frame's scene pixels (ptrt_internal.h FrameParams::scene_x0 ..): a rectangle of pixels outside of which no camera ray can hit
// anything, so that those pixels' samples need no tracing (kernels.hip k_sky_pixels). Returns whether the image has such a pixel; if not,
// or if nothing can be said, the rectangle is everything.
//   The box: the union of the root node's child boxes as the device holds them (a ray reaches a triangle only through the slab test of
// one of them) and of every sphere's box, the radius taken as sqrt(r^2 + 2^-16 (|c - o| + r)^2): sphere_test's discriminant b^2 - (|oc|^2
// - r^2) carries a rounding error of about 13 * 2^-24 |oc|^2 (three roundings in each dot product, the ray's direction normalised to 3
// ulp), so a ray that passes a small far sphere at several radii can still be accepted. Each side then moves out by 1e-4 of the largest
// coordinate in play (box, camera origin): the slab test's t = fma(plane, inv, -(o * inv)) is off by at most 3 * 2^-24 (|o| + |plane|)
// in units of the plane's position, the quantised layouts' fused form and the 1.0000004 on the far side by as little.
//   The projection: camera_vec's map inverted, v = a right + b up + c forward, pixel = ((a / c + cx) / scale, (b / c + cy) / scale), in
// double, of the box's 8 corners; their bounding rectangle (the box is convex and in front of the camera plane) widened by one pixel and
// by 1e-4 of the image's size and principal point, against the 2^-24 relative roundings of camera_vec and normalize. A pixel is a scene
// pixel unless its footprint [x, x + 1) x [y, y + 1) lies outside that. Everything is a scene pixel if a corner has c <= 1e-4 (|a| + |b| +
// |c|) (beside or behind the camera plane, or the camera inside the box), if the basis is near-singular, scale is not positive, a
// coordinate is beyond 1e15 (the slab test's 1e20 reciprocals would overflow) or the tree's bound is stale.
bool scene_pixels(const pt_scene *s, const pt_camera &cam, uint32_t W, uint32_t H, FrameParams &fp)
{
    fp.scene_x0 = fp.scene_y0 = 0u; fp.scene_x1 = fp.scene_y1 = ~0u;
    Box tb;
    if (!s->tree.root_bound(tb)) return false;
    double lo[3], hi[3], o[3], big = 0.0;
    for (int k = 0; k < 3; ++k) { lo[k] = tb.lo[k]; hi[k] = tb.hi[k]; o[k] = cam.origin[k]; big = std::max(big, std::fabs(o[k])); }
    for (size_t i = 0; i < s->sph_mat.size(); ++i) {
        const float *sp = &s->spheres[i * 4];
        const double r = sp[3], dx = sp[0] - o[0], dy = sp[1] - o[1], dz = sp[2] - o[2], reach = std::sqrt(dx * dx + dy * dy + dz * dz) + r;
        const double rr = std::sqrt(r * r + std::ldexp(reach * reach, -16));
        for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], sp[k] - rr); hi[k] = std::max(hi[k], sp[k] + rr); }
    }
    if (!(lo[0] <= hi[0])) { fp.scene_x0 = fp.scene_x1 = fp.scene_y0 = fp.scene_y1 = ~0u; return true; } // nothing to hit: every pixel is sky
    for (int k = 0; k < 3; ++k) big = std::max(big, std::max(std::fabs(lo[k]), std::fabs(hi[k])));
    if (!(big < 1e15)) return false;
    for (int k = 0; k < 3; ++k) { lo[k] -= 1e-4 * big; hi[k] += 1e-4 * big; }
    const double R[3] = { cam.right[0], cam.right[1], cam.right[2] }, U[3] = { cam.up[0], cam.up[1], cam.up[2] }, F[3] = { cam.forward[0], cam.forward[1], cam.forward[2] };
    auto cross = [](const double *a, const double *b, double *c) { c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0]; };
    auto dot = [](const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
    double UF[3], FR[3], RU[3];
    cross(U, F, UF); cross(F, R, FR); cross(R, U, RU);
    const double det = dot(R, UF), scale = cam.scale;
    if (!(std::fabs(det) > 1e-6 * std::sqrt(dot(R, R) * dot(U, U) * dot(F, F))) || !(scale > 0.0) || !std::isfinite(scale)) return false;
    double x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
    for (int i = 0; i < 8; ++i) {
        const double v[3] = { ((i & 1) ? hi[0] : lo[0]) - o[0], ((i & 2) ? hi[1] : lo[1]) - o[1], ((i & 4) ? hi[2] : lo[2]) - o[2] };
        const double a = dot(v, UF) / det, b = dot(v, FR) / det, c = dot(v, RU) / det;
        if (!(c > 1e-4 * (std::fabs(a) + std::fabs(b) + std::fabs(c)))) return false;
        const double px = (a / c + cam.cx) / scale, py = (b / c + cam.cy) / scale;
        x0 = std::min(x0, px); x1 = std::max(x1, px); y0 = std::min(y0, py); y1 = std::max(y1, py);
    }
    const double mx = 1.0 + 1e-4 * ((double)W + std::fabs(cam.cx / scale)), my = 1.0 + 1e-4 * ((double)H + std::fabs(cam.cy / scale));
    x0 -= mx; x1 += mx; y0 -= my; y1 += my;
    if (!std::isfinite(x0) || !std::isfinite(x1) || !std::isfinite(y0) || !std::isfinite(y1)) return false;
    // pixel x is sky iff x + 1 <= x0 or x >= x1: x < floor(x0) or x >= ceil(x1)
    auto px_of = [](double v, uint32_t n) { return (uint32_t)std::min(std::max(v, 0.0), (double)n); };
    fp.scene_x0 = px_of(std::floor(x0), W); fp.scene_x1 = px_of(std::ceil(x1), W);
    fp.scene_y0 = px_of(std::floor(y0), H); fp.scene_y1 = px_of(std::ceil(y1), H);
    if (fp.scene_x0 == 0u && fp.scene_x1 >= W && fp.scene_y0 == 0u && fp.scene_y1 >= H) { fp.scene_x1 = fp.scene_y1 = ~0u; return false; }
    return true;
}

// pt_stats.reserved[3] of a frame that resolved sky pixels (include/ptrt.h): the rectangle scene_pixels left to be traced, 16 bits a side;
// all ones if it holds no pixel (every pixel was resolved); 0 for an image with a side beyond 65535, which has no such code.
uint64_t scene_pixels_code(const FrameParams &fp)
{
    if (fp.scene_x0 >= fp.scene_x1 || fp.scene_y0 >= fp.scene_y1) return ~0ull;
    if (fp.width > 0xFFFFu || fp.height > 0xFFFFu) return 0ull;
    return (uint64_t)fp.scene_x0 | (uint64_t)fp.scene_x1 << 16 | (uint64_t)fp.scene_y0 << 32 | (uint64_t)fp.scene_y1 << 48;
}

// The aperture's axes of a frame through a lens (docs/SPEC.md §3.1), in f32 with §0's dot: radius * right / |right| and radius * up / |up| of
// the frame's camera. False for a degenerate basis: a zero dot product, or a component that is not finite.
bool lens_basis(const pt_camera &cam, const pt_lens &lens, LensArgs &out)
{
    auto dot = [](const float *a) { return std::fma(a[2], a[2], std::fma(a[1], a[1], a[0] * a[0])); };
    const float dr = dot(cam.right), du = dot(cam.up);
    if (dr == 0.0f || du == 0.0f) return false;
    const float ru = lens.radius * (1.0f / std::sqrt(dr)), rv = lens.radius * (1.0f / std::sqrt(du));
    for (int k = 0; k < 3; ++k) {
        out.u[k] = cam.right[k] * ru; out.v[k] = cam.up[k] * rv;
        if (!std::isfinite(out.u[k]) || !std::isfinite(out.v[k])) return false;
    }
    out.focus = lens.focus_distance; out.pad = 0u;
    return true;
}

// The lens domain (docs/SPEC.md §3.1 "Domain"): whether normalize's dot(w, w) of w = F v - a is a normal, finite f32 for every pixel,
// jitter and point on the lens of a W x H frame. In double, from the camera's f32 words:
//   n    = cross(right, up): the normal of the plane that holds a and the sx, sy terms of v; refused unless |n| > 2^-6 |right| |up|
//   vmax = max over the image's corners (x = 0 or W, y = 0 or H) of |v|, each sx and sy moved outwards by 2^-22 (W |scale| + |cx|), the
//          f32 roundings of §3's sx (|v| is convex in (sx, sy), so its largest value over the image is at a corner)
//   hi   = F vmax + R sqrt(1 + |dot(right, up)| / (|right| |up|))       >= |w|: |a|^2 <= R^2 (lx^2 + ly^2) (1 + |cos|)
//   S    = |forward| + (max |sx| + |cx| + W |scale|) |right| + (max |sy| + |cy| + H |scale|) |up|: the size of the terms v is summed from
//   lo   = F (|dot(forward, n)| / |n| - 2^-11 S)                        <= |w|, see below
//   accepted iff lo >= 2^-60 and hi^2 <= 2^127.
// Only forward leaves the plane, so the exact |w| is at least F |dot(forward, n)| / |n|; the f32 w is off by at most 4 u F S (v, u = 2^-24)
// plus 25 u r R (a, for a lens point at radius r) plus u |w|. With |a| >= k r R, k = sqrt(1 - |cos|) >= 2^-6.5: either k r R <= 2 F S,
// and the error is at most (4 + 50 / k) u F S < 2^-11 F S; or |a| > 2 F S >= 2 F |v|, and |w| >= |a| / 2 - error > F S (1 - 2^-10).
// dot(w, w) then lies in [2^-120, 2^127] up to its own roundings: a factor 2 below the overflow, 2^6 above the subnormals, where a
// product that underflows loses less than 2^-30 of the sum. Anything not finite fails a comparison and is refused.
bool lens_in_domain(const pt_camera &cam, const pt_lens &lens, uint32_t W, uint32_t H)
{
    const double r[3] = { cam.right[0], cam.right[1], cam.right[2] }, u[3] = { cam.up[0], cam.up[1], cam.up[2] }, f[3] = { cam.forward[0], cam.forward[1], cam.forward[2] };
    auto dot = [](const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
    const double n[3] = { r[1] * u[2] - r[2] * u[1], r[2] * u[0] - r[0] * u[2], r[0] * u[1] - r[1] * u[0] };
    const double nn = std::sqrt(dot(n, n)), lr = std::sqrt(dot(r, r)), lu = std::sqrt(dot(u, u)), F = lens.focus_distance, R = lens.radius;
    if (!(nn > 0x1p-6 * lr * lu)) return false;
    const double scale = cam.scale, cx = cam.cx, cy = cam.cy, tw = (double)W * std::fabs(scale) + std::fabs(cx), th = (double)H * std::fabs(scale) + std::fabs(cy);
    const double ax = -cx, bx = (double)W * scale - cx, ay = -cy, by = (double)H * scale - cy;
    const double sxs[2] = { std::min(ax, bx) - std::ldexp(tw, -22), std::max(ax, bx) + std::ldexp(tw, -22) };
    const double sys[2] = { std::min(ay, by) - std::ldexp(th, -22), std::max(ay, by) + std::ldexp(th, -22) };
    double vmax = 0.0;
    for (int i = 0; i < 4; ++i) {
        const double sx = sxs[i & 1], sy = sys[i >> 1];
        const double v[3] = { f[0] + sx * r[0] + sy * u[0], f[1] + sx * r[1] + sy * u[1], f[2] + sx * r[2] + sy * u[2] };
        const double len = std::sqrt(dot(v, v));
        if (!std::isfinite(len)) return false;
        vmax = std::max(vmax, len);
    }
    const double hi = F * vmax + R * std::sqrt(1.0 + std::fabs(dot(r, u)) / (lr * lu));
    const double S = std::sqrt(dot(f, f)) + (std::max(std::fabs(ax), std::fabs(bx)) + tw) * lr + (std::max(std::fabs(ay), std::fabs(by)) + th) * lu;
    const double lo = F * (std::fabs(dot(f, n)) / nn - std::ldexp(S, -11));
    return lo >= 0x1p-60 && hi * hi <= 0x1p127;
}

struct Frame {                  // a path-traced frame as plan_frame lays it out, and what its loops leave for finish_frame
    uint32_t nranks, streams, pixel_slots, n_slots, shard_cap, samples_per_stream, lag, n_loops, packed_chunk, default_bounces;
    Pipeline pipe;              // what the frame's flags, pt_tuning.extend_kernel and the scene decode to (pipeline.h)
    bool accumulate, mapped, compact;
    NeeArgs nee_args; EnvArgs env_args; LensArgs lens_args; // the blocks of a pipe.nee / pipe.env / pipe.lens frame
    SphArgs sph_args;           // ... and of a pipe.sph frame, whose nee_args holds the joint table (docs/SPEC.md §7.1)
    TexArgs tex_args;           // ... and of a pipe.tex frame (docs/SPEC.md §13)
    bool sky;                   // the frame has sky pixels (scene_pixels) and resolves them at its start instead of tracing their paths
    Accumulation::Key sums_key; // what the sums hold once this frame completes
    size_t q_entries; uint64_t total_spp, allocs_before;
    PathState ps; FrameParams fp;
    uint32_t iters; uint64_t slot_launches; size_t n_events; // launches of the longest loop, paths alive at launch starts, profile events
    std::vector<uint64_t> trace_alive, trace_rays;
};

} // namespace

// (the frame's stream `q`; ps and fp are the frame's, with the template's own queue and counter block put in place of the frame's)
pt_status FrameTemplate::build_if_differs(pt_context *c, hipStream_t q, Key key, const Pipeline &pipe, const DeviceScene &ds, const PathState &ps,
                                          const FrameParams &fp, const QueueSizes &sizes)
{
    key.q = q_init.p;
    if (valid && key == key_) return PT_OK;
    valid = false; HIP_TRY(c, hipMemsetAsync(cnt_init.p, 0, sizeof(uint32_t) * kCntTotalWords, q));
    PathState pt = ps; pt.counters = cnt_init.p; pt.q_ext[0] = q_init.p;
    // whole streams without a sample (spp < streams): the first queue holds the live slots only, and the first launch is sized by it
    const bool dense = key.first_spp < key.streams;
    HIP_TRY(c, launch_generate(q, ds, pt, fp, pipe.generate_mode(dense))); // also zeroes every slot's sum unless the frame accumulates
    bound = key.shard_cap;
    if (dense) {
        uint32_t *h = sizes.template_sizes();
        HIP_TRY(c, hipMemcpyAsync(h, cnt_init.p, sizeof(uint32_t) * kShards * kCounterStride, hipMemcpyDeviceToHost, q));
        HIP_TRY(c, hipStreamSynchronize(q));
        bound = 0;
        for (uint32_t sh = 0; sh < kShards; ++sh) bound = std::max(bound, h[cnt_ext_index(0, sh)]);
    }
    key_ = key; valid = true;
    return PT_OK;
}

// What a frame's flags, the context's tuning and the scene decode to (pipeline.h), and what its sums will hold: one statement each for
// plan_frame and for the refusals pt_render makes before the frame is replaced.
static PipelineDecode decode_frame(const pt_context *c, const pt_scene *s, const pt_render_params *p)
{
    return decode_pipeline(p->flags, c->tuning.extend_kernel, s->env.present(), s->has_specular, s->lens.radius > 0.f, s->n_sph_lights != 0u, s->textures.textured());
}
static Accumulation::Key sums_key_of(const pt_render_params *p)
{
    return Accumulation::Key{ p->width, p->height, p->rank, p->nranks ? p->nranks : 1u, p->streams ? p->streams : 1u, p->seed,
                              (p->flags & PT_FLAG_NEXT_EVENT) != 0, (p->flags & PT_FLAG_NEXT_EVENT_SPHERES) != 0 };
}
static pt_status other_light_set(pt_context *c)
{
    return fail(c, PT_ERR_INVALID_ARGUMENT, "PT_FLAG_ACCUMULATE: the sums so far were made %s PT_FLAG_NEXT_EVENT_SPHERES", c->sums.sphere_lights() ? "with" : "without");
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
    const PipelineDecode d = decode_frame(c, s, p);
    if (d.status != PT_OK) return fail(c, d.status, "%s", d.message);
    const Pipeline &pipe = f.pipe = d.pipeline;
    if (pipe.lens && !lens_basis(s->ds.cam, s->lens, f.lens_args))
        return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_render through a lens: the camera's right or up has length 0, or the aperture's axes are not finite");
    f.mapped = t.readback == 0u; // queue sizes reach the host by the kernels' own stores (fold_traced) instead of a copy per launch
    // rays per wavefront of the lane-packing kernel: 256 once several sample streams keep the queues long, else 128 (measured)
    f.packed_chunk = t.packed_chunk >= 64u ? t.packed_chunk : (f.streams >= 4u ? 256u : 128u);
    // path vertices per launch of the one-ray-per-lane kernel: 3/4 max_depth - 2 (saturating), clamped to [4, 12]
    const uint32_t v34 = p->max_depth * 3u / 4u; f.default_bounces = std::min(12u, std::max(4u, v34 > 2u ? v34 - 2u : 0u));
    // NEE: `bounces` counts rays, and a vertex with a light sample takes two (shadow, then extension): twice the passes for about as many
    // vertices per launch
    if (pipe.nee) f.default_bounces *= 2u;
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
    f.sums_key = sums_key_of(p);
    if (f.accumulate)
        switch (c->sums.continues(f.sums_key, p->sample_offset)) {
        case Accumulation::Refusal::other_frame:
            return fail(c, PT_ERR_INVALID_ARGUMENT, "PT_FLAG_ACCUMULATE needs a previous frame with the same size, rank, nranks, streams and seed");
        case Accumulation::Refusal::other_estimator:
            return fail(c, PT_ERR_INVALID_ARGUMENT, "PT_FLAG_ACCUMULATE: the sums so far were made %s PT_FLAG_NEXT_EVENT", c->sums.next_event() ? "with" : "without");
        case Accumulation::Refusal::other_light_set: return other_light_set(c);
        case Accumulation::Refusal::wrong_offset:
            return fail(c, PT_ERR_INVALID_ARGUMENT, "PT_FLAG_ACCUMULATE: sample_offset must be %llu (samples so far)", (unsigned long long)c->sums.samples());
        case Accumulation::Refusal::none: break;
        }
    f.total_spp = (f.accumulate ? c->sums.samples() : 0u) + p->spp; c->sums.begin(); // the sums: invalid until this frame completes
    f.allocs_before = g_device_allocs;
    HIP_TRY(c, c->ray_o.ensure(f.n_slots)); HIP_TRY(c, c->ray_d.ensure(f.n_slots)); HIP_TRY(c, c->thr.ensure(f.n_slots));
    HIP_TRY(c, c->acc.ensure(f.n_slots)); HIP_TRY(c, c->out.tiles.ensure(f.pixel_slots)); HIP_TRY(c, c->sd.ensure(f.n_slots));
    HIP_TRY(c, c->q_ext0.ensure(f.q_entries)); HIP_TRY(c, c->q_ext1.ensure(f.q_entries));
    // hit records and the metal / dielectric buckets are k_shade's (no kernel indexes the miss and Lambert buckets)
    if (pipe.split) { HIP_TRY(c, c->hit.ensure(f.n_slots)); HIP_TRY(c, c->q_metal.ensure(f.q_entries)); HIP_TRY(c, c->q_dielectric.ensure(f.q_entries)); }
    if (!pipe.full_state()) HIP_TRY(c, c->start.reserve(f.q_entries));
    const uint32_t ovf = s->tree.stack_overflow();
    if (ovf) HIP_TRY(c, c->stack_ovf.ensure((size_t)ovf * f.q_entries));
    if (pipe.nee) {
        HIP_TRY(c, c->nee_ext.ensure(f.n_slots)); HIP_TRY(c, c->nee_rad.ensure(f.n_slots));
        f.nee_args = NeeArgs{ s->d_lights.p, s->d_cdf.p, s->d_pa.p, s->n_lights, c->nee_ext.p, c->nee_rad.p };
        if (pipe.sph) { // §7.1: "the table" is the joint table
            f.nee_args = NeeArgs{ s->d_jlights.p, s->d_jcdf.p, s->d_jpa.p, s->n_lights + s->n_sph_lights, c->nee_ext.p, c->nee_rad.p };
            f.sph_args = SphArgs{ s->d_sph_pmf.p, s->n_lights, 0u };
        }
    }
    // §11: a light sample picks one of the two kinds of light with probability 1/2 when the frame has both
    if (pipe.env) f.env_args = s->env.args(pipe.nee && s->env.lit() && (s->n_lights || pipe.sph) ? 0.5f : 1.0f);
    if (pipe.tex) f.tex_args = s->textures.args();
    if (f.nranks == 1) HIP_TRY(c, c->out.resize(p->width, p->height));
    PathState &ps = f.ps;
    ps.ray_o = c->ray_o.p; ps.ray_d = c->ray_d.p; ps.thr = c->thr.p; ps.sd = c->sd.p; ps.acc = c->acc.p; ps.q_ext[0] = c->q_ext0.p; ps.q_ext[1] = c->q_ext1.p;
    if (pipe.split) { ps.hit = c->hit.p; ps.q_bucket[B_METAL] = c->q_metal.p; ps.q_bucket[B_DIELECTRIC] = c->q_dielectric.p; }
    ps.counters = c->counters.p; ps.stack_ovf = c->stack_ovf.p; ps.stack_ovf_entries = ovf; ps.n_slots = f.n_slots; ps.shard_cap = f.shard_cap;
    ps.shard_base = 0; ps.shard_count = kShards; ps.compact_below = t.compact_below; ps.finish_below = t.finish_below; ps.sparse_below = t.sparse_below;
    ps.repack_sticky = (f.samples_per_stream <= t.sticky_samples && t.compact_below > 0.f) ? 1u : 0u;
    ps.host_ring = c->sizes.begin(f.mapped); ps.ring_slots = kLag;
    f.compact = pipe.forces_compact(ps.repack_sticky != 0u, f.samples_per_stream);
    FrameParams &fp = f.fp;
    fp.width = p->width; fp.height = p->height; fp.spp = p->spp; fp.max_depth = p->max_depth; fp.rr_start = p->rr_start;
    fp.seed_hashed = host_pcg(p->seed); fp.sample_offset = p->sample_offset; fp.ray_eps = p->ray_eps;
    fp.rank = p->rank; fp.nranks = f.nranks; fp.tiles_x = lay.tiles_x; fp.n_tiles = lay.n_tiles; fp.streams = f.streams; fp.slots_per_stream = f.pixel_slots;
    div_magic(f.streams, fp.streams_magic, fp.streams_shift); div_magic(lay.tiles_x, fp.tiles_x_magic, fp.tiles_x_shift);
    fp.offset_mod = p->sample_offset % f.streams; fp.accumulate = f.accumulate ? 1u : 0u;
    fp.scene_x0 = fp.scene_y0 = 0u; fp.scene_x1 = fp.scene_y1 = ~0u;
    f.sky = pipe.resolves_sky() && scene_pixels(s, s->ds.cam, p->width, p->height, fp);
    return PT_OK;
}

// Start: the first extend queue and counter block, after ev_start. A full-state frame runs k_generate over every slot; a fused one copies the
// template of its geometry (context.h FrameTemplate: k_generate's output depends on which slots exist and on whether every stream has a sample).
static pt_status start_frame(pt_context *c, const pt_scene *s, const pt_render_params *p, const Frame &f)
{
    hipStream_t q = c->stream; const bool full_state = f.pipe.full_state();
    if (full_state) {
        HIP_TRY(c, hipMemsetAsync(c->counters.p, 0, sizeof(uint32_t) * kCntTotalWords, q));
        HIP_TRY(c, hipEventRecord(c->ev_start, q));
        HIP_TRY(c, launch_generate(q, s->ds, f.ps, f.fp, f.pipe.generate_mode(false)));
    } else {
        HIP_TRY(c, hipEventRecord(c->ev_start, q));
        FrameTemplate::Key key{};
        key.w = p->width; key.h = p->height; key.rank = p->rank; key.nranks = f.nranks; key.streams = f.streams; key.first_spp = std::min(p->spp, f.streams);
        key.offset = f.fp.offset_mod; key.n_slots = f.n_slots; key.shard_cap = f.shard_cap; key.acc = c->acc.p;
        const pt_status st = c->start.build_if_differs(c, q, key, f.pipe, s->ds, f.ps, f.fp, c->sizes);
        if (st != PT_OK) return st;
        HIP_TRY(c, hipMemcpyAsync(c->counters.p, c->start.counters(), sizeof(uint32_t) * kCntTotalWords, hipMemcpyDeviceToDevice, q));
        // the template is the geometry's, not the camera's: it still queues the sky pixels' slots, and the first launch leaves them out
        if (f.sky) HIP_TRY(c, launch_sky_pixels(q, s->ds, f.ps, f.fp));
    }
    c->start.frame_ran(f.accumulate || full_state); // the template invariant: this frame writes the streams a dense template leaves out
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
    hipStream_t q = c->stream; const Pipeline &pipe = f.pipe; const bool full_state = pipe.full_state();
    const uint32_t n_loops = f.n_loops, per_group = kShards / n_loops;
    struct Loop { hipStream_t stream; uint32_t base, bound, iters; bool done; } loops[kMaxGroups];
    HIP_TRY(c, hipEventRecord(c->ev_fork, q));
    for (uint32_t g = 0; g < n_loops; ++g) {
        loops[g] = Loop{ n_loops == 1 ? q : c->group_stream[g], g * per_group, full_state ? f.shard_cap : c->start.first_bound(), 0u, false }; // no shard's queue can outgrow its first one
        if (loops[g].stream != q) HIP_TRY(c, hipStreamWaitEvent(loops[g].stream, c->ev_fork, 0));
    }
    const uint64_t max_iters = (uint64_t)p->spp * p->max_depth * (pipe.nee ? 2u : 1u) + kLag + 2; // NEE: up to two rays per vertex
    const bool trace = pipe.profile && getenv("PTRT_TRACE") != nullptr; // developer aid: per-iteration table on stderr
    for (uint32_t live = n_loops; live > 0;) {
        for (uint32_t g = 0; g < n_loops; ++g) {
            Loop &L = loops[g];
            if (L.done) continue;
            if (L.iters >= max_iters) return fail(c, PT_ERR_INTERNAL, "wavefront loop did not drain after %u iterations", L.iters);
            const uint32_t it = L.iters; PathState pg = f.ps; pg.shard_base = L.base; pg.shard_count = per_group;
            if (it == 0u && !full_state) pg.q_ext[0] = c->start.first_queue(); // the frame's first queue is the template: read, never written
            if (x.kernel == 0u) pg.finish_below = 0u; // probing: no finish mode
            hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
            if (pipe.profile) {
                e0 = pool_event(c, f.n_events++); e1 = pool_event(c, f.n_events++); e2 = pool_event(c, f.n_events++);
                if (!e0 || !e1 || !e2) return fail(c, PT_ERR_HIP, "hipEventCreate failed"); // (the text this failure has always had)
                HIP_TRY(c, hipEventRecord(e0, L.stream));
            }
            const bool probing = x.probing(g, it); const ExtendKernel kernel = pipe.kernel_for(x.kernel, probing ? it : 0u);
            if (probing) HIP_TRY(c, hipEventRecord(c->ev_probe[(it - 2u) * 2u], L.stream));
            const ExtendLaunch launch{ it, L.bound, kernel, pipe.fuse(), pipe.count, f.compact, f.packed_chunk,
                                       c->tuning.bounces ? c->tuning.bounces : x.bounces(g, it, kernel, f.default_bounces),
                                       pipe.nee ? &f.nee_args : nullptr, pipe.env ? &f.env_args : nullptr, pipe.lens ? &f.lens_args : nullptr,
                                       pipe.sph ? &f.sph_args : nullptr, pipe.tex ? &f.tex_args : nullptr };
            HIP_TRY(c, launch_extend(L.stream, s->ds, pg, f.fp, launch));
            if (pipe.profile) HIP_TRY(c, hipEventRecord(e1, L.stream));
            if (pipe.bucket) {
                HIP_TRY(c, launch_shade(L.stream, s->ds, pg, f.fp, it, L.bound, SHADE_QUEUE, true));
                HIP_TRY(c, launch_shade(L.stream, s->ds, pg, f.fp, it, L.bound, SHADE_BUCKETS, true)); // metal + dielectric buckets
            } else if (pipe.split) HIP_TRY(c, launch_shade(L.stream, s->ds, pg, f.fp, it, L.bound, pipe.shade, f.compact));
            if (probing) HIP_TRY(c, hipEventRecord(c->ev_probe[(it - 2u) * 2u + 1u], L.stream)); // the whole iteration, either way
            if (pipe.profile) HIP_TRY(c, hipEventRecord(e2, L.stream));
            HIP_TRY(c, c->sizes.post(L.stream, g, it, c->counters.p + cnt_ext_index((it + 1u) % 3u, L.base), per_group));
            f.iters = std::max(f.iters, ++L.iters);
            if (L.iters < f.lag) continue;
            const uint32_t old_iter = L.iters - f.lag; // iteration old_iter traced `traced` rays and left `total` paths alive: its survivors bound every later queue
            QueueSizes::Sizes left;
            HIP_TRY(c, c->sizes.wait(g, old_iter, L.base, per_group, left));
            const uint64_t total = left.alive, traced = left.traced;
            L.bound = left.longest;
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
    HIP_TRY(c, launch_reduce_streams(q, c->acc.p, c->out.tiles.p, f.pixel_slots, f.streams)); // tiles = the pixel sums = the gather payload
    if (f.nranks == 1)
        HIP_TRY(c, launch_assemble(q, c->out.tiles.p, 1, f.pixel_slots, p->width, p->height, fp.tiles_x, fp.n_tiles, 1.0f / (float)f.total_spp, c->out.fb.p, c->out.fb8.p));
    HIP_TRY(c, hipEventRecord(c->ev_stop, q));
    HIP_TRY(c, hipMemcpyAsync(c->sizes.frame_end(), c->counters.p, sizeof(uint32_t) * kCntTotalWords, hipMemcpyDeviceToHost, q));
    HIP_TRY(c, hipStreamSynchronize(q));
    pt_stats out{}; const CounterView hc{ c->sizes.frame_end(), 0u };
    if (hc.error()) return fail(c, PT_ERR_INTERNAL, "device error flag 0x%x (1 = traversal stack overflow, 2 = step limit)", hc.error());
    for (uint32_t sh = 0; sh < kShards; ++sh) {
        if (hc.word(cnt_alive_index(0, sh)) || hc.word(cnt_alive_index(1, sh)) || hc.word(cnt_alive_index(2, sh))) return fail(c, PT_ERR_INTERNAL, "extend queue of shard %u not empty at frame end", sh);
        out.rays += hc.u64(cnt_rays_index(sh));
    }
    float ms = 0.f; HIP_TRY(c, hipEventElapsedTime(&ms, c->ev_start, c->ev_stop)); out.gpu_ms = ms;
    out.node_visits = hc.u64(kCntNodes); out.tri_tests = hc.u64(kCntTris); out.sphere_tests = hc.u64(kCntSph);
    // PT_FLAG_COUNT_VISITS + one-ray-per-lane kernel: wave-level node-loop iterations (bits 0-39) and, from bit 40 up, how many
    // of them came after the wave's first leaf phase of the ray (diagnostic for tools/exp_util.py)
    out.reserved[3] = (hc.u64(kCntWaveNodeIters) & 0xFFFFFFFFFFull) | (hc.u64(kCntWaveNodeIters + 2) << 40);
    if (f.sky) out.reserved[3] = scene_pixels_code(fp); // (a frame that resolves sky pixels never counts: the counters above are 0)
    if (f.pipe.count && getenv("PTRT_TRACE")) { // developer aid: where the node loop's lane-slots go (one-ray-per-lane kernel)
        const double slots = 64.0 * (double)hc.u64(kCntWaveNodeIters), v = (double)out.node_visits, lf = (double)hc.u64(kCntIdleLeaf), dn = (double)hc.u64(kCntIdleDone);
        if (slots > 0) fprintf(stderr, "ptrt: node-loop lane-slots %.3g: visiting %.1f %%, waiting at a leaf %.1f %%, ray finished %.1f %%, no ray %.1f %%\n", slots,
                               100 * v / slots, 100 * lf / slots, 100 * dn / slots, 100 * (slots - v - lf - dn) / slots);
    }
    out.iterations = f.iters; out.extend_launches = f.iters;
    x.frame_done(out.rays, out.gpu_ms, g_device_allocs != f.allocs_before); // (the rays the extend kernels traced: resolved sky pixels join below)
    out.reserved[0] = x.kernel ? x.kernel : (uint32_t)EXT_SIMPLE; // extend kernel in use at frame end (ExtendKernel)
    out.reserved[1] = hc.word(kCntCompactions); // (shard, iteration) pairs that re-packed their queue (the others carried it over in place)
    uint64_t px = 0, scene_px = 0; // paths = owned in-image pixels x spp; scene_px: those of them inside the frame's scene rectangle
    for (uint32_t t = p->rank; t < fp.n_tiles; t += f.nranks) {
        const uint32_t tx = t % fp.tiles_x, ty = t / fp.tiles_x;
        const uint32_t xa = tx * kTile, ya = ty * kTile, xb = xa + std::min(kTile, p->width - xa), yb = ya + std::min(kTile, p->height - ya);
        px += (uint64_t)(xb - xa) * (yb - ya);
        const int64_t ix = (int64_t)std::min(xb, fp.scene_x1) - (int64_t)std::max(xa, fp.scene_x0), iy = (int64_t)std::min(yb, fp.scene_y1) - (int64_t)std::max(ya, fp.scene_y0);
        scene_px += (uint64_t)(std::max<int64_t>(ix, 0) * std::max<int64_t>(iy, 0));
    }
    out.paths = px * p->spp;
    // every sample of a sky pixel is one camera ray that k_sky_pixels resolved instead of the extend kernels tracing (and counting) it
    out.rays += (px - scene_px) * p->spp;
    // path states read + written by the wavefront loop = sum over launches of the paths alive at launch start
    // (iteration 0 starts every (pixel, stream) pair that has a sample)
    out.reserved[2] = f.slot_launches + px * std::min(f.streams, p->spp);
    if (f.pipe.profile) {
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
        if (trace && f.sky) fprintf(stderr, "ptrt: sky pixels x [%u, %u) y [%u, %u) excepted: %llu of %llu pixels, %llu rays resolved at frame start\n", fp.scene_x0,
                                    fp.scene_x1, fp.scene_y0, fp.scene_y1, (unsigned long long)(px - scene_px), (unsigned long long)px, (unsigned long long)((px - scene_px) * p->spp));
    }
    c->out.tiles_hold(f.pixel_slots); c->sums.complete(f.sums_key, f.total_spp);
    if (f.nranks == 1) c->out.complete(FrameOutputs::Holds::path_traced);
    if (stats) *stats = out;
    return PT_OK;
}

static pt_status render_frame(pt_context *c, const pt_scene *s, const pt_render_params *p, pt_stats *stats)
{
    if (!c || !p) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_render: NULL argument");
    pt_tile_layout lay; pt_status st = layout_of(p, &lay);
    if (st != PT_OK) return fail(c, st, "pt_render: bad width/height/rank/nranks/tile_size");
    HIP_TRY(c, hipSetDevice(c->device));
    c->out.replace(); // the denoised results belong to the frame this call replaces
    if (p->mode == PT_REFERENCE_SPHERE) { // Renderer.ComputeFrame: one dispatch, then the host blocks on the fence (Renderer.cs:1020,1036,972)
        HIP_TRY(c, c->out.resize(p->width, p->height));
        HIP_TRY(c, hipEventRecord(c->ev_start, c->stream));
        HIP_TRY(c, launch_reference_sphere(c->stream, p->width, p->height, c->out.fb.p, c->out.fb8.p));
        HIP_TRY(c, hipEventRecord(c->ev_stop, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        float ms = 0.f; HIP_TRY(c, hipEventElapsedTime(&ms, c->ev_start, c->ev_stop));
        pt_stats out{};
        out.gpu_ms = ms; out.other_ms = ms; out.rays = out.paths = (uint64_t)p->width * p->height; out.iterations = 1;
        c->out.complete(FrameOutputs::Holds::reference_sphere); if (stats) *stats = out;
        return PT_OK;
    }
    if (p->mode != PT_PATH_TRACE) return fail(c, PT_ERR_INVALID_ARGUMENT, "unknown mode %u", p->mode);
    Frame f{};
    if ((st = plan_frame(c, s, p, lay, f)) != PT_OK) return st;
    ExtendFrame x(s->cache.ext, f.pipe);
    f.n_loops = f.pipe.single_loop(x.kernel == 0u) ? 1u : c->tuning.loops ? c->tuning.loops : 2u;
    if ((st = start_frame(c, s, p, f)) != PT_OK || (st = run_loops(c, s, p, f, x)) != PT_OK) return st;
    return finish_frame(c, p, f, x, stats);
}

extern "C" pt_status pt_render(pt_context *c, const pt_scene *s, const pt_render_params *p, pt_stats *stats)
{
    // A lens outside its domain (lens_in_domain) is refused here, before the call begins to replace the frame: the framebuffer, the sums of
    // a PT_FLAG_ACCUMULATE sequence, the denoised, temporal and displayed results and the history all stay. Every other refusal is render_frame's.
    if (c && s && p && p->mode == PT_PATH_TRACE && s->ctx == c && s->committed && s->lens.radius > 0.f && !lens_in_domain(s->ds.cam, s->lens, p->width, p->height))
        return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_render through a lens: the lens (radius %g, focus_distance %g) is outside its domain for this camera and a %u x %u image "
                    "(docs/SPEC.md 3.1: focus_distance * |v| + radius too large, focus_distance * forward's part off the plane of right and up too small, or no such plane)",
                    (double)s->lens.radius, (double)s->lens.focus_distance, p->width, p->height);
    // So are the refusals of sphere lights (docs/SPEC.md §7.1), by plan_frame's own two rules (which it then finds met): what a frame with
    // PT_FLAG_NEXT_EVENT_SPHERES decodes to — the bit without PT_FLAG_NEXT_EVENT, a pipeline that next-event estimation refuses — and
    // PT_FLAG_ACCUMULATE over sums that differ from this frame's in the setting of the bit alone.
    if (c && s && p && p->mode == PT_PATH_TRACE && s->ctx == c && s->committed) {
        if (p->flags & PT_FLAG_NEXT_EVENT_SPHERES) {
            const PipelineDecode d = decode_frame(c, s, p);
            if (d.status != PT_OK) return fail(c, d.status, "%s", d.message);
        }
        if ((p->flags & PT_FLAG_ACCUMULATE) && c->sums.continues(sums_key_of(p), p->sample_offset) == Accumulation::Refusal::other_light_set) return other_light_set(c);
    }
    const pt_status st = drained_on_failure(c, [&] { return render_frame(c, s, p, stats); });
    if (st != PT_OK && c) { c->sums.begin(); c->out.lost(); } // nothing of this frame survives the call
    return st;
}
