// ptrt_internal.h — structs shared by the host API (api.cpp) and the kernel launchers (kernels.hip).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include "../../include/ptrt.h"
#include "pipeline.h"

namespace ptrt {

constexpr uint32_t kTileShift = 6;                 // 64x64 tiles (docs/SPEC.md §6)
constexpr uint32_t kTile = 1u << kTileShift;
constexpr uint32_t kTilePixels = kTile * kTile;
constexpr uint32_t kBlock = 256;                   // threads per workgroup = 4 wavefronts
#ifndef PT_SHARD_GROUP_SHIFT
#define PT_SHARD_GROUP_SHIFT 6
#endif
// Consecutive slots that share a shard: 2^this. 64 = one wavefront: consecutive wavefronts (the sample streams of one 8x8 pixel
// block) go to consecutive shards, i.e. to different XCDs, and every shard gets an even cut of every tile. Measured, ms per frame
// with groups of 64 / 256 / 512 / 1024 / 4096 slots: headline 17.91 / 18.01 / 18.29 / 18.18 / 18.70; a rank's 1/8 of it 2.65 / 2.72 /
// 2.71 / 2.62 / 3.16; 512 spp 135.9 / 137.1 / 138.5 / 139.0 / 142.2; glass 256 spp 38.9 / 39.1 / 39.5 / 39.8 / 40.7; soup ±0.5 %.
constexpr uint32_t kShardGroupShift = PT_SHARD_GROUP_SHIFT;
#ifndef PT_STACK_LDS
#define PT_STACK_LDS 12
#endif
#ifndef PT_EXT_BLOCK
#define PT_EXT_BLOCK 64
#endif
constexpr uint32_t kStackLds = PT_STACK_LDS;       // traversal-stack entries kept in LDS per lane
constexpr uint32_t kExtBlock = PT_EXT_BLOCK;       // workgroup size of k_extend (a wave retires on its own when it is 64)
constexpr uint32_t kMaxSpheres = 64;
// Largest grid of k_trace (pt_trace_rays), in one-wave workgroups: 2^20 lanes = two rounds of the 8192 waves an MI355X holds at 8 waves
// per SIMD. Every lane keeps one overflow-stack column for the whole batch, so this bounds the overflow area of a query.
constexpr uint32_t kTraceBlocks = 16384;
#ifndef PT_POOL
#define PT_POOL 128
#endif
constexpr uint32_t kPool = PT_POOL;                // queue entries per wavefront of k_extend_pool (64 P)

// Queue sharding. A slot belongs to one shard for the whole frame — k_generate (kernels.hip) deals the groups of 2^kShardGroupShift slots
// out in rotation: slot group g goes to shard (g % kShards + g / kShards) % kShards, as entry group g / kShards —, every queue is kShards
// independent regions of `shard_cap` entries with one counter line each, and a workgroup works on exactly one shard
// (kernels.hip block_pos: 1-D grids with the shard as the fastest index).
// Why: a queue push is one returning atomic per wavefront; on ONE address that saturates at ~88 atomics/us
// (MI355X_MICROARCH.md "dequeue"), which made both wavefront kernels atomic-bound (~230 us per launch regardless of
// the scene). 64 counters on 64 separate lines take the same pushes at ~64x the rate.
constexpr uint32_t kShards = 64;
constexpr uint32_t kCounterStride = 16;            // u32 words between counters: one 64-B line each

enum Bucket : uint32_t { B_MISS = 0, B_LAMBERT = 1, B_METAL = 2, B_DIELECTRIC = 3, B_COUNT = 4 };

// counters block (u32 words). ext[iteration % 3][shard], bucket[parity][bucket][shard], rays[shard] (u64), then globals.
constexpr uint32_t kCntExt = 0;
constexpr uint32_t kCntBucket = kCntExt + 3 * kShards * kCounterStride;
constexpr uint32_t kCntRays = kCntBucket + 2 * B_COUNT * kShards * kCounterStride;
constexpr uint32_t kCntGlobals = kCntRays + kShards * kCounterStride;
constexpr uint32_t kCntError = kCntGlobals + 0;
constexpr uint32_t kCntNodes = kCntGlobals + 2, kCntTris = kCntGlobals + 4, kCntSph = kCntGlobals + 6; // u64 each
constexpr uint32_t kCntCompactions = kCntGlobals + 8; // (shard, iteration) pairs that re-packed their queue
constexpr uint32_t kCntWaveNodeIters = kCntGlobals + 10; // u64, PT_FLAG_COUNT_VISITS: iterations of the wave-level node loop of k_extend
// u64 x 3, PT_FLAG_COUNT_VISITS, one-ray-per-lane kernel: lane-slots of the node loop spent (a) waiting at a leaf for the wave's node loop,
// (b) with the ray already finished, (c) without a ray at all (hole, ended stream); the rest of 64 x iterations made a node visit
constexpr uint32_t kCntIdleLeaf = kCntGlobals + 16, kCntIdleDone = kCntGlobals + 18, kCntIdleDead = kCntGlobals + 20;
constexpr uint32_t kCntTotalWords = kCntGlobals + 24;

// An extend queue has LEN entries of which ALIVE hold a slot; the rest are kInvalidSlot holes left by paths that ended
// while the queue was carried over in place (k_shade, compact == 0). Both counts share the shard's 64-B line.
constexpr uint32_t kInvalidSlot = 0xFFFFFFFFu;
inline __host__ __device__ uint32_t cnt_ext_index(uint32_t parity, uint32_t shard) { return kCntExt + (parity * kShards + shard) * kCounterStride; }
inline __host__ __device__ uint32_t cnt_alive_index(uint32_t parity, uint32_t shard) { return cnt_ext_index(parity, shard) + 1u; }
// third word of the line: rays traced by the iteration that FILLED this queue; the next iteration folds it into rays[shard]
// word 4 of the line: alive entries at the start of the launch that FILLED this queue (written by that launch's first thread)
inline __host__ __device__ uint32_t cnt_prev_alive_index(uint32_t parity, uint32_t shard) { return cnt_ext_index(parity, shard) + 4u; }
inline __host__ __device__ uint32_t cnt_traced_index(uint32_t parity, uint32_t shard) { return cnt_ext_index(parity, shard) + 2u; }
inline __host__ __device__ uint32_t cnt_bucket_index(uint32_t parity, uint32_t bucket, uint32_t shard)
{
    return kCntBucket + ((parity * B_COUNT + bucket) * kShards + shard) * kCounterStride;
}
inline __host__ __device__ uint32_t cnt_rays_index(uint32_t shard) { return kCntRays + shard * kCounterStride; }

struct DeviceScene {
    const float4 *nodes;   // BVH-N: node i slot c = rows (i*N + c)*2 + {0: lo.xyz|ref, 1: hi.xyz|0}
    const float4 *tris;    // 4 rows (one 64-B line) per triangle, blob order: v0|orig_id, e1|material, e2|0, then the
                           // shading row normalize(cross(e1,e2))|material
    const float4 *spheres; // cx,cy,cz,r
    const uint2 *sph_mat;  // per sphere: material id, bits of 1.0f / r (the IEEE quotient, made once at commit: the shading step's own division gone)
    const float4 *mats;    // 3 rows per material (48 B pt_material)
    uint32_t n_nodes, n_tris, n_spheres, n_mats;
    float sky[3];
    uint32_t bvh_width;
    pt_camera cam;
};

struct PathState {           // SoA over slots
    float4 *ray_o;           // o.xyz, -
    float4 *ray_d;           // d.xyz, -
    float2 *hit;             // t, ref bits
    float4 *thr;             // T.rgb, key bits
    uint32_t *sd;            // sample << 8 | depth
    float4 *acc;             // radiance sum rgb, path count
    uint32_t *q_ext[2];      // extend queues (slot ids) [shard][shard_cap], by iteration parity
    uint32_t *q_bucket[B_COUNT]; // shade queues per material kind, [shard][shard_cap]
    uint32_t *counters;
    int32_t *stack_ovf;      // traversal stack overflow, [entry][kShards * shard_cap]
    uint32_t stack_ovf_entries;
    uint32_t n_slots;
    uint32_t shard_cap;      // entries per shard region = slots owned by a shard (multiple of 2^kShardGroupShift)
    uint32_t shard_base, shard_count; // the shards this launch covers: shard_base .. + shard_count (groups of shards run as
                                      // independent wavefront loops on their own streams, see api.cpp)
    // queue policy, decided on the device from the shard's own counters (no host lag):
    float compact_below;     // re-pack a shard's queue when the alive/length ratio it would leave is below this (> 1: always, 0: never)
    uint32_t repack_sticky;  // this frame has few samples per stream: a shard that has re-packed once re-packs in every launch (want_compact)
    float sparse_below;      // fused one-ray-per-lane kernel: a launch that starts with alive < sparse_below * length advances one
                             // vertex only (and re-packs), instead of running `bounces` vertices on mostly idle wavefronts
    uint32_t finish_below;   // fused kernel: once a shard has no more alive paths than this, a launch runs them to their end
    // Queue sizes for the host, without a copy dispatch between two launches: the first thread of shard s in launch `it` stores the line
    // the PREVIOUS launch left behind (queue length, alive entries, rays it traced) to host_ring[((it - 1) % ring_slots) * kShards + s]
    // — host-mapped pinned memory; the host reads it after the event that follows launch `it`. NULL: the host copies the lines itself.
    uint4 *host_ring;
    uint32_t ring_slots;
};

// Next-event estimation (PT_FLAG_NEXT_EVENT, docs/SPEC.md §7): the light table of the committed scene (api.cpp build_lights) and the
// per-slot state a pending shadow ray leaves behind. A separate block behind ExtArgs (kernels.hip ExtArgsT) rather than fields of
// DeviceScene / PathState: those sit in the kernarg segment of every extend kernel, and growing them would move the offsets every other
// kernel loads its arguments from.
struct NeeArgs {
    const float4 *lights;  // 4 rows per light, in light order: v0|pa, e1|Le.r, e2|Le.g, n_l|Le.b (pa = pmf / area, n_l = the shading row)
    const float *cdf;      // n_lights entries, the last one 1.0f
    const float *pa;       // per blob triangle: pa of the light it is, 0 for every other triangle (read on emissive hits only)
    uint32_t n_lights;
    float4 *ext;           // per slot, while a shadow ray is pending: the extension ray's direction | its Lambert pdf
    float4 *rad;           // per slot, while a shadow ray is pending: the radiance the shadow ray adds if it reaches the light | -
};

// The environment map of a scene (pt_scene_set_environment, docs/SPEC.md §11; environment.cpp builds and uploads the table). Like
// NeeArgs a block of its own behind ExtArgs / NeeArgs (kernels.hip ExtArgsT), for the same reason; only the environment
// instantiations of k_extend have it.
struct EnvArgs {
    const float4 *texels;  // n * n records, row-major: r, g, b, p (the texel's pdf over the unit square of the map, x n * n / 4)
    const float *mcdf;     // n entries: the marginal cdf over rows, the last one 1.0f
    const float *ccdf;     // n * n entries: row j's conditional cdf over columns, the last one of every row 1.0f
    uint32_t n;
    float nf, step;        // (float)n, 2.0f / (float)n
    uint32_t lit;          // the table's total is positive: the environment is a light for PT_FLAG_NEXT_EVENT frames
    float psel;            // this frame's probability of the strategy a light sample takes: 0.5f with both kinds of light, else 1.0f
};

// The thin lens of a scene (pt_scene_set_lens, docs/SPEC.md §3.1) as a frame's camera rays use it: the aperture's two axes, made by
// frame.cpp from the frame's camera (lens_basis), and the focus distance. A block of its own at the end of the lens instantiations'
// arguments (kernels.hip ExtLensArgsT), for the reason NeeArgs gives; only those instantiations have it.
struct LensArgs {
    float u[3], v[3];      // lens_u = radius * right / |right|, lens_v = radius * up / |up|
    float focus;           // F: every lens ray of a sample passes through origin + F * v (v: §3's vector before it is normalised)
    uint32_t pad;
};
static_assert(sizeof(LensArgs) == 32, "LensArgs is 32 bytes");

// Sphere lights (PT_FLAG_NEXT_EVENT_SPHERES / PT_GATHER_PATHS_SPHERE_LIGHTS, docs/SPEC.md §7.1) on a scene that has one. The call's NeeArgs
// then holds the JOINT table (scene.cpp build_sphere_lights): §7's triangle lights with the joint pa, then the sphere lights, whose 4 rows
// are centre|pmf, (r, bits of 1 + its sphere index, -)|Le.r, -|Le.g, -|Le.b; NeeArgs::pa is the joint per-triangle pa. This block is what the sphere side adds, at
// the very end of the arguments of the instantiations that have it (kernels.hip ExtSphArgsT, GatherSphArgsT), for the reason NeeArgs gives.
struct SphArgs {
    const float *pmf;      // per sphere of the scene: pmf of the light it is in the joint table, 0 for every other sphere (read on emissive hits only)
    uint32_t n_tri;        // the joint table's entries [0, n_tri) are triangles, [n_tri, n_lights) spheres
    uint32_t pad;
};
static_assert(sizeof(SphArgs) == 16, "SphArgs is 16 bytes");

// Albedo textures (docs/SPEC.md §13) of a textured scene, as scene.cpp's SceneTextures builds them at commit. A block of its own at the very
// end of the arguments of the instantiations that have it (kernels.hip ExtTexArgsT; denoise.hip k_guide_resolve_tex takes it as a last
// parameter), not fields of DeviceScene or PathState, for the reason NeeArgs gives: those two sit at the front of every extend kernel's
// kernarg segment, and a field more would move every offset behind it in kernels that never see a texture.
// uv: two rows per BLOB triangle, {s0, t0, s1, t1}, {s2, t2, bits of the descriptor index of the triangle's material or PT_NO_TEXTURE, 0}:
// the material is resolved to its texture at commit, so the chain hit -> uv rows -> descriptor -> texels runs beside hit -> shading row ->
// material instead of behind it. desc: one row per texture that is set and bound, {first texel, width, height, flags}. texels: every such
// texture's width * height float4 {r, g, b, 0} in one allocation.
struct TexArgs {
    const float4 *uv;
    const uint4 *desc;
    const float4 *texels;
    uint32_t n_desc;       // rows of desc (a descriptor index in uv is below it, or PT_NO_TEXTURE)
    uint32_t pad;
};
static_assert(sizeof(TexArgs) == 32, "TexArgs is 32 bytes");

struct FrameParams {
    uint32_t width, height, spp, max_depth, rr_start, seed_hashed, sample_offset;
    float ray_eps;
    uint32_t rank, nranks, tiles_x, n_tiles;
    uint32_t streams;          // K sample streams per pixel (docs/SPEC.md §5); slot <-> (pixel slot, stream): kernels.hip slot_of()
    uint32_t slots_per_stream; // pixel slots of this rank (tiles_per_rank * 4096)
    uint32_t accumulate;       // PT_FLAG_ACCUMULATE: keep the partial sums of the previous frame(s)
    // Division by `streams` and by `tiles_x` (slot -> pixel, once per regenerated path) as multiply-high + shift: a 32-bit division by a
    // run-time value is ~22 instructions, five of them quarter-rate integer multiplies, and the regeneration code runs in practically
    // every bounce of every wave. q = umulhi(n, magic) >> shift is exact for n < 2^31 (magic = ceil(2^(31 + l) / d), shift = l - 1,
    // l = ceil(log2 d)); magic 0 stands for d == 1. div_magic() below makes the pair on the host.
    uint32_t streams_magic, streams_shift, tiles_x_magic, tiles_x_shift;
    uint32_t offset_mod;       // sample_offset % streams
    // The frame's scene pixels: x in [scene_x0, scene_x1) and y in [scene_y0, scene_y1). No camera ray of a pixel outside can hit anything
    // (frame.cpp scene_pixels), so its samples are all the sky: k_sky_pixels sums them at frame start and the fused extend kernels'
    // first launch does not start its slots. (0, ~0, 0, ~0): every pixel may see the scene, nothing is resolved.
    uint32_t scene_x0, scene_x1, scene_y0, scene_y1;
};
inline __host__ __device__ bool sky_pixel(const FrameParams &fp, uint32_t x, uint32_t y)
{
    return x < fp.scene_x0 || x >= fp.scene_x1 || y < fp.scene_y0 || y >= fp.scene_y1;
}
inline void div_magic(uint32_t d, uint32_t &magic, uint32_t &shift)
{
    if (d <= 1u) { magic = 0u; shift = 0u; return; }
    uint32_t l = 0; while ((1ull << l) < d) ++l;
    magic = (uint32_t)(((1ull << (31u + l)) + d - 1u) / d); shift = l - 1u;
}
inline __host__ __device__ uint32_t div_by(uint32_t n, uint32_t magic, uint32_t shift)
{
    return magic ? (uint32_t)(((uint64_t)n * magic) >> 32) >> shift : n; // the high half of a 32 x 32 multiply: v_mul_hi_u32 on the device
}

// kernel launchers (kernels.hip). All enqueue on `s` and return the launch error.
// `shard_bound` = upper bound of any shard's queue length for this launch.
hipError_t launch_reference_sphere(hipStream_t s, uint32_t w, uint32_t h, float4 *out_f, uint32_t *out_rgba8);
hipError_t launch_generate(hipStream_t s, const DeviceScene &sc, const PathState &ps, const FrameParams &fp, GenerateMode mode);
// The frame's sky pixels (FrameParams::scene_x0 ..), once per frame before the first extend launch: every sample of their slots added
// to the slot's sum as the traced frame would have. Their rays, one per sample, are the host's to count (frame.cpp finish_frame).
hipError_t launch_sky_pixels(hipStream_t s, const DeviceScene &sc, const PathState &ps, const FrameParams &fp);
// One launch of an extend kernel. `it` = iteration index of the wavefront loop: queues alternate by it & 1, queue counters rotate by it % 3.
// (kernel, fuse, count, nee, env, lens, sph, tex) must name an instantiation that exists (pipeline.h extend_instantiated), else hipErrorInvalidValue.
struct ExtendLaunch {
    uint32_t it, shard_bound;   // shard_bound: upper bound of any shard's queue length for this launch
    ExtendKernel kernel; ShadeMode fuse; bool count, compact; // compact (fused kernels): as for launch_shade
    uint32_t packed_chunk;      // queue entries per wavefront of EXT_PACKED
    uint32_t bounces;           // fused only: path vertices a lane advances per launch
    const NeeArgs *nee;         // a PT_FLAG_NEXT_EVENT frame's block, else NULL
    const EnvArgs *env;         // the block of a scene with an environment map, else NULL
    const LensArgs *lens;       // the block of a frame through a thin lens (radius > 0), else NULL
    const SphArgs *sph = nullptr; // the block of a PT_FLAG_NEXT_EVENT_SPHERES frame on a scene with a sphere light (nee: the joint table), else NULL
    const TexArgs *tex = nullptr; // the block of a textured scene (docs/SPEC.md §13), else NULL
};
hipError_t launch_extend(hipStream_t s, const DeviceScene &sc, const PathState &ps, const FrameParams &fp, const ExtendLaunch &x);
// mode: SHADE_QUEUE, SHADE_BUCKETS or SHADE_INLINE (pipeline.h)
// compact: 1 = survivors are appended densely to the next queue (ballot + one returning atomic per wavefront);
//          0 = every lane writes its own position of the next queue (slot or kInvalidSlot): no returning atomics, and the
//              queue keeps its slot order, which is what keeps the slot-indexed path state coalesced (SHADE_QUEUE and SHADE_INLINE only)
hipError_t launch_shade(hipStream_t s, const DeviceScene &sc, const PathState &ps, const FrameParams &fp, uint32_t it, uint32_t shard_bound, ShadeMode mode, bool compact);
// pt_trace_rays: n <= 2^31 caller rays (2 float4 rows each) -> hit records (1 float4 row each), on a grid of trace_blocks(n) workgroups of
// kExtBlock lanes. ps: only counters (error word and visit counters at kCntGlobals), stack_ovf, stack_ovf_entries and shard_cap are read;
// shard_cap * kShards must cover trace_blocks(n) * kExtBlock lanes. occlusion and count are exclusive.
uint32_t trace_blocks(uint32_t n);
hipError_t launch_trace(hipStream_t s, const DeviceScene &sc, const PathState &ps, const float4 *rays, float4 *hits, uint32_t n, bool occlusion, bool count);
// pt_gather (docs/SPEC.md §12): n <= 2^31 caller points (2 float4 rows each) -> 2 float4 rows each, a group of 2^gather_group_shift(samples)
// lanes per point on a grid of gather_blocks(n, samples) workgroups of kExtBlock lanes. ps as for launch_trace; shard_cap * kShards must
// cover the grid's lanes. The kernel adds the invalid points it met to the low word of kCntNodes. env (may be NULL): the scene's map.
// pp (NULL for pt_gather): the call is pt_gather_paths (§12.1), the same points, grid and counters; every sample is a path of §5 of at most
// max_depth (1..255) segments with Russian roulette from rr_start on. The kernel adds the segments it traced to the u64 at kCntTris.
// nee (NULL, or with pp): PT_GATHER_PATHS_NEXT_EVENT (§12.2) on a scene that has a light: the light table (ext and rad are not used), and
// with it env->psel and env->lit as a NEE frame sets them. The shadow rays are counted with the segments.
// sph (NULL, or with nee): PT_GATHER_PATHS_SPHERE_LIGHTS (§7.1) on a scene that has a sphere light; nee is then the joint table.
struct GatherParams {
    uint32_t samples, seed, point_offset, sample_offset; // samples in 1..4096
    float tmax, ray_eps;                                        // tmax: max_distance, +inf for "unbounded"
};
struct GatherPathParams { uint32_t max_depth, rr_start; };
uint32_t gather_group_shift(uint32_t samples); // log2 of min(64, the power of two >= samples)
uint32_t gather_blocks(uint32_t n, uint32_t samples);
hipError_t launch_gather(hipStream_t s, const DeviceScene &sc, const PathState &ps, const float4 *points, float4 *out, uint32_t n, const GatherParams &gp,
                         const GatherPathParams *pp, const EnvArgs *env, const NeeArgs *nee = nullptr, const SphArgs *sph = nullptr);
hipError_t launch_reduce_streams(hipStream_t s, const float4 *acc, float4 *tiles, uint32_t slots_per_stream, uint32_t streams);
hipError_t launch_assemble(hipStream_t s, const float4 *gathered, uint32_t nranks, uint32_t slots_per_rank,
                           uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t n_tiles, float inv_spp,
                           float4 *fb, uint32_t *fb8);

// api.cpp: what comm.cpp needs to know about a context
int context_device(const pt_context *c);
hipStream_t context_stream(const pt_context *c);
void context_set_error(pt_context *c, const char *msg); // c == NULL: the calling thread's last error

// lbvh.hip: Morton sort + Karras hierarchy + refit on the device; returns the binary tree on the host
struct BinaryBvh;
struct DeviceBlob4Q;
hipError_t build_lbvh_device(hipStream_t s, const float *verts9, uint32_t n_tris, BinaryBvh &out);
// the same, packed into the BVH4Q blob + triangle records on the device (only the few-thousand-box top storey visits the host)
hipError_t build_lbvh_blob4q_device(hipStream_t s, const float *verts9, const uint32_t *mats, uint32_t n_tris, DeviceBlob4Q &out);

} // namespace ptrt
