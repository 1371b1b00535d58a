/*
 * ptrt.h — C ABI of libptrt.so, the MI355X (gfx950) wavefront path tracer that stands where the
 * reference's Vulkan compute path stands.
 *
 * The reference (chairclr/PathTracing) has no plugin/FFI interface; its de-facto seam is the private trio
 *   Renderer.CreateResources      RayTracing/Graphics/Renderer.cs:105-196   (W x H RGBA image)
 *   Renderer.CreateComputePipeline RayTracing/Graphics/Renderer.cs:293-403  (load Test.spirv, bind image)
 *   Renderer.ComputeFrame(delta)  RayTracing/Graphics/Renderer.cs:1006-1040 (CmdDispatch + QueueSubmit)
 * plus the fence wait in Renderer.Render (Renderer.cs:970-972). Contract of the seam: "after ComputeFrame
 * and the fence wait, a W x H RGBA image owned by the renderer holds the frame". Each entry point below
 * names the reference code it replaces. The P/Invoke stub a maintainer would add is in INTEGRATION.md.
 *
 * Conventions (mirroring the reference's behaviour):
 *  - every call returns pt_status (0 = ok); nothing throws or aborts across the ABI. The C#/C++/Python host
 *    wrappers turn non-zero into an exception, as every Vulkan failure does in the reference
 *    (e.g. Renderer.cs:1022-1025, 1036-1039).
 *  - a pt_context is single-caller; pt_render is synchronous (returns after the stream is idle), like the
 *    host-side fence wait at Renderer.cs:972.
 *  - host arrays passed in are borrowed for the call only; output buffers are caller-allocated.
 *  - all structs are plain little-endian f32/u32, blittable.
 *  - there is NO CPU backend: without a gfx950 device pt_context_create fails with PT_ERR_NO_DEVICE.
 */
#ifndef PTRT_H
#define PTRT_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* 2: pt_tuning grew to 40 bytes (extend_kernel, readback); pt_comm_*, pt_framebuffer_read_srgb8, PT_FLAG_EXTEND_POOL, pt_bvh_info.stack_need and
 * the BVH2 default for small scenes had arrived under version 1. pt_trace_rays and PT_TRACE_* arrived later under version 2, and after them
 * pt_scene_update_triangles / pt_scene_update_spheres and PT_UPDATE_HOST_MEMORY, then PT_FLAG_NEXT_EVENT, then pt_denoise, pt_denoise_params,
 * PT_DENOISE_*, pt_denoised_read / pt_denoised_device_ptr and pt_guides_read, then pt_denoise_temporal, pt_temporal_params, PT_TEMPORAL_*,
 * pt_temporal_read / pt_temporal_device_ptr / pt_temporal_history_read, then pt_display, pt_display_params, pt_display_info, PT_DISPLAY_*,
 * PT_TONE_*, pt_display_read / pt_display_device_ptr / pt_display_info_read / pt_display_histogram_read, then PT_TEMPORAL_MOTION, then
 * pt_scene_set_environment, pt_environment_info and pt_scene_environment_info / pt_scene_environment_read, then pt_gather, pt_gather_params and
 * PT_GATHER_HOST_MEMORY, then pt_lens and pt_scene_set_lens / pt_scene_get_lens, then pt_gather_paths and pt_gather_path_params,
 * then PT_GATHER_PATHS_NEXT_EVENT, then PT_FLAG_NEXT_EVENT_SPHERES and PT_GATHER_PATHS_SPHERE_LIGHTS, then pt_scene_set_triangle_uvs,
 * pt_scene_set_texture, pt_scene_set_material_textures, pt_texture_info and pt_scene_texture_info (additions only: no struct or existing
 * signature changed).
 * Hosts compare pt_abi_version() with the header they were built against. */
#define PTRT_ABI_VERSION 2

typedef int32_t pt_status;
enum {
    PT_OK = 0,
    PT_ERR_INVALID_ARGUMENT = 1,
    PT_ERR_NO_DEVICE = 2,      /* no HIP device / not gfx950 */
    PT_ERR_HIP = 3,            /* a HIP runtime call failed; text in pt_last_error */
    PT_ERR_OUT_OF_MEMORY = 4,
    PT_ERR_NOT_COMMITTED = 5,  /* scene used before pt_scene_commit */
    PT_ERR_UNSUPPORTED = 6,
    PT_ERR_INTERNAL = 7
};

typedef struct pt_context pt_context; /* opaque; owns the device, stream, path-state queues, framebuffer */
typedef struct pt_scene pt_scene;     /* opaque; owns host copies, the BVH and the device scene */

/* modes of pt_render */
enum {
    PT_REFERENCE_SPHERE = 0, /* exact Test.hlsl:1-40 semantics (docs/SPEC.md §1) */
    PT_PATH_TRACE = 1        /* wavefront path tracer (docs/SPEC.md §2-§6) */
};
/* material kinds */
enum { PT_LAMBERT = 0, PT_METAL = 1, PT_DIELECTRIC = 2 };
/* pt_render_params.flags */
enum {
    PT_FLAG_PROFILE_KERNELS = 1u, /* bracket every kernel with HIP events on the context's stream; fills pt_stats.*_ms */
    PT_FLAG_COUNT_VISITS = 2u,    /* count BVH node visits / triangle / sphere tests on the device (slower build of extend) */
    PT_FLAG_EXTEND_PACKED = 4u,   /* force the lane-packing extend kernel (a wavefront owns a chunk of the queue and refills idle lanes by ballot) */
    PT_FLAG_EXTEND_SIMPLE = 8u,   /* force the one-ray-per-lane extend kernel. Neither flag: probed per scene (pt_stats.reserved[0]) */
    PT_FLAG_BUCKET_SPECULAR = 32u, /* shade metal / dielectric hits from per-kind bucket queues (wave-uniform BSDF code) instead of
                                     in queue order. Slower on MI355X: re-queued slots scramble the queue order and state access
                                     loses its coalescing; kept for comparison (implies PT_FLAG_SPLIT_KERNELS) */
    PT_FLAG_SPLIT_KERNELS = 64u,  /* run extend and shade as two kernels per iteration (hit records through HBM) instead of shading
                                     inside the extend kernel; same frame, lets PT_FLAG_PROFILE_KERNELS time the two separately */
    PT_FLAG_EXTEND_POOL = 128u,   /* force the pooled extend kernel (a wavefront owns 128 queue entries, refills idle lanes during
                                     traversal and shades the whole pool at full width) */
    PT_FLAG_ACCUMULATE = 16u,    /* progressive rendering: keep the sums of the previous call(s) (same size/rank/streams/seed and
                                     PT_FLAG_NEXT_EVENT / _SPHERES setting, sample_offset = samples so far) and show the mean over all samples — the
                                     converging analogue of the reference's render-every-frame loop (App.cs:39-42) */
    PT_FLAG_NEXT_EVENT = 256u,    /* next-event estimation (docs/SPEC.md §7): every Lambert vertex also samples a point on an emissive triangle
                                     and traces a shadow ray to it, combined with the BSDF-sampled hits by multiple importance sampling. Same
                                     mean, far less noise in scenes lit by small emitters. The BSDF-sampled paths are those of a plain frame;
                                     pt_stats.rays then counts their rays plus the shadow rays traced. Runs on the one-ray-per-lane kernel:
                                     with PT_FLAG_EXTEND_PACKED / _POOL, PT_FLAG_SPLIT_KERNELS / _BUCKET_SPECULAR, pt_tuning.extend_kernel 2 / 3
                                     or PT_FLAG_COUNT_VISITS the frame is PT_ERR_UNSUPPORTED */
    PT_FLAG_NEXT_EVENT_SPHERES = 512u /* with PT_FLAG_NEXT_EVENT (alone: PT_ERR_INVALID_ARGUMENT): the scene's emissive spheres join the light set
                                     (docs/SPEC.md §7.1). A light sample that picks one draws a direction in the cone the sphere subtends from
                                     the vertex, and a hit of such a sphere by a ray that left a Lambert vertex is weighted against that pdf.
                                     Same mean again; far less noise where a small emissive sphere (a bulb) lights the scene. On a scene
                                     without an emissive sphere the frame is the PT_FLAG_NEXT_EVENT frame bit for bit. Refuses what
                                     PT_FLAG_NEXT_EVENT refuses */
};
/* pt_scene_commit options */
enum {
    PT_BVH_WIDTH_DEFAULT = 0, /* PT_BVH_WIDTH_4Q; PT_BVH_WIDTH_2 for scenes of at most 192 triangles (pt_bvh_info.width tells) */
    PT_BVH_WIDTH_2 = 2,       /* binary, 64-B nodes, f32 child boxes */
    PT_BVH_WIDTH_4 = 4,       /* 4-wide, 128-B nodes, f32 child boxes */
    PT_BVH_WIDTH_4Q = 68,     /* 4-wide, 64-B nodes, child boxes quantised to 8 bits on a per-node power-of-two grid */
    PT_BVH_WIDTH_8Q = 72,     /* 8-wide, one 128-B cache line per node (96 B used), the same quantisation: a node visit costs the
                                 memory system one line either way, and there are fewer visits */
    PT_BVH_WIDTH_8O = 73,     /* the 128-B node of PT_BVH_WIDTH_8Q with the children placed in slots by the octant of the node they lie in:
                                 visited in the order slot ^ (sign bits of the ray direction), no distance sort (docs/SPEC.md §4.1) */
    PT_BVH_BUILD_LBVH = 0x100 /* OR-ed onto a layout: build the hierarchy on the GPU (Morton sort + Karras + refit) instead of the
                                 host's binned-SAH builder. Faster to build, slower to trace; the picture is identical either way. */
};

typedef struct {
    int32_t device_ordinal; /* hipSetDevice argument; the reference picks its device in GraphicsDevice.cs:38-43 */
    void *stream;           /* an existing hipStream_t to run on, or NULL to create one */
    uint32_t flags;         /* reserved, 0 */
    uint32_t reserved;
} pt_device_desc;

typedef struct { uint32_t kind; float albedo[3]; float emission[3]; float roughness; float ior; uint32_t pad[3]; } pt_material; /* 48 B */
/* Accepted by pt_scene_set_materials: kind <= PT_DIELECTRIC, finite fields, roughness in [0, 1] and, for a dielectric,
 * PT_IOR_MIN <= ior <= PT_IOR_MAX (2^-20 .. 2^20): the range in which eta*eta is finite and the formulas of docs/SPEC.md §5 give a
 * finite direction at every incidence, on both sides of the surface. ior is not looked at for the other kinds. */
#define PT_IOR_MIN 9.5367431640625e-07f /* 2^-20 */
#define PT_IOR_MAX 1048576.0f           /* 2^20 */

/* pinhole camera, docs/SPEC.md §3. The reference's literal camera (Test.hlsl:6-10) is
 * origin (0,0,1), forward (0,0,-1), right (1,0,0), up (0,1,0), scale 2/1080, cx = cy = 1, jitter 0
 * up to the +0.5 pixel centre that Test.hlsl omits. */
typedef struct { float origin[3], forward[3], right[3], up[3]; float scale, cx, cy; uint32_t jitter; } pt_camera; /* 64 B */

typedef struct {
    uint32_t width, height;  /* frame size; the reference hard-codes 1920x1080 (App.cs:27, Renderer.cs:1020) */
    uint32_t spp;            /* samples per pixel (reference: 1 ray per pixel, Test.hlsl) */
    uint32_t max_depth;      /* max path segments */
    uint32_t rr_start;       /* Russian roulette from this depth on */
    uint32_t seed;
    uint32_t sample_offset;  /* first sample index (progressive accumulation across calls) */
    uint32_t mode;           /* PT_REFERENCE_SPHERE | PT_PATH_TRACE */
    float ray_eps;           /* origin offset along the normal for continuation rays */
    uint32_t rank, nranks;   /* image-space partition: this process renders tiles t with t % nranks == rank */
    uint32_t tile_size;      /* 0 = 64 */
    uint32_t flags;          /* PT_FLAG_* */
    uint32_t streams;        /* sample streams per pixel kept in flight at once (docs/SPEC.md §5): sample s goes to stream
                                s mod streams, each stream has its own partial sum, the pixel is their fixed-order sum.
                                0 = 1; at most 64. More streams = more rays per wavefront iteration, same picture definition. */
    uint32_t pad[2];
} pt_render_params; /* 64 B */

typedef struct {
    uint64_t rays;          /* ray-scene intersection queries = path segments (the benchmark's unit); with PT_FLAG_NEXT_EVENT plus the
                               shadow rays traced, so that rays(NEE) - rays(plain) of the same frame is the shadow-ray count */
    uint64_t paths;
    uint64_t node_visits, tri_tests, sphere_tests; /* only with PT_FLAG_COUNT_VISITS, else 0 */
    uint32_t iterations;    /* wavefront iterations = launches of the extend kernel; the default (fused one-ray-per-lane) kernel advances
                               every path by up to 3/4 max_depth - 2 clamped to [4, 12] vertices per iteration, the lane-packing one by up
                               to 64 (pt_tuning.bounces overrides) */
    uint32_t extend_launches;
    double gpu_ms;          /* hipEvent start->stop around all kernels of the frame */
    double extend_ms;       /* sum of extend-kernel durations (PT_FLAG_PROFILE_KERNELS); includes shading when fused */
    double shade_ms;        /* sum of shade-kernel durations  (PT_FLAG_PROFILE_KERNELS); ~0 when fused */
    double other_ms;        /* generate / resolve kernels */
    uint64_t reserved[4];   /* diagnostics: [0] extend kernel in use (1 one ray per lane, 2 lane-packing, 3 pooled, 0 unprobed),
                               [1] iterations that re-packed their queues, [2] path states loaded+stored by the loop
                               (sum over iterations of the paths alive at its start), [3] with PT_FLAG_COUNT_VISITS: wave-level
                               iterations of k_extend's node loop in bits 0-39 (node_visits / (64 * that) = lane utilisation of the
                               loop), those after the wave's first leaf phase from bit 40 up; without that flag: the pixels the
                               frame traced, where it resolved the others as sky at its start: 0 = nothing was resolved, else the
                               rectangle x0 | x1 << 16 | y0 << 32 | y1 << 48 of pixels x0 <= x < x1, y0 <= y < y1 that were still
                               traced (every pixel outside it was resolved), or all ones where every pixel was resolved (the
                               rectangle is empty). Images with a side beyond 65535 report 0 */
} pt_stats;

typedef struct {
    uint32_t width;          /* the layout id the scene was committed with: PT_BVH_WIDTH_2, _4, _4Q, _8Q or _8O */
    uint32_t n_nodes;
    uint32_t n_tris;
    uint32_t max_depth;
    uint64_t node_bytes;     /* n_nodes * 64 (layouts 2 and 4Q) or n_nodes * 128 (layouts 4, 8Q and 8O) */
    uint64_t tri_bytes;      /* n_tris * 48: the blob's triangle records as pt_scene_bvh_read copies them out (docs/SPEC.md §4.1). On the device
                                every record is padded to one 64-byte line (+ a shading row): n_tris * 64 bytes of HBM */
    double build_ms;
    float sah_cost;
    uint32_t stack_need;     /* worst-case traversal-stack depth of this tree (entries); the kernels keep 12 per lane in LDS and
                                size a global overflow area from this */
} pt_bvh_info;

/* Scheduling knobs of a context (none changes a pixel; tests/test_gpu_parity.py holds every setting to the same frame). Read the
 * current values with pt_context_get_tuning, change what you want, write them back. The library reads no environment variables for
 * these (developer aids aside: the stderr diagnostics PTRT_TRACE / PTRT_TIMING, which change no tree and no picture). */
typedef struct {
    uint32_t bounces;       /* path vertices a lane advances per launch of the fused extend kernels, 1..64; 0 (default) = 3/4 max_depth - 2
                               clamped to [4, 12] for the one-ray-per-lane kernel, 64 for the lane-packing one. PT_FLAG_NEXT_EVENT frames:
                               rays (shadow or extension) a lane traces per launch; 0 = twice the one-ray-per-lane default */
    uint32_t loops;         /* independent shard-group wavefront loops per frame, each on its own stream: 1, 2 or 4; 0 (default) = two
                               (frames with PT_FLAG_PROFILE_KERNELS / PT_FLAG_COUNT_VISITS always run one: their kernels are timed alone) */
    uint32_t finish_below;  /* a shard with at most this many live paths runs them to their end in one launch (default 4096; 0 = never) */
    uint32_t packed_chunk;  /* queue entries per wavefront of the lane-packing kernel, >= 64; 0 (default) = 256 with >= 4 streams, else 128 */
    float compact_below;    /* a shard re-packs its queue in a launch that would otherwise leave alive < this * length behind (default 0.9;
                               > 1 every launch; 0 never) */
    float sparse_below;     /* one-ray-per-lane kernel: a launch that starts with alive < this * length advances one vertex only (default 0 = off) */
    uint32_t sticky_samples; /* frames with at most this many samples per stream (spp / streams): a shard that has re-packed once re-packs
                               in every launch, and with at most 2 samples per stream every launch re-packs (default 32; 0 = off) */
    uint32_t lag;           /* wavefront iterations the host runs ahead of the queue sizes it reads back: 2..5; 0 (default) = 3 for frames
                               of at most 2 samples per stream, else 4 (one less each with readback = 1) */
    uint32_t extend_kernel; /* 0 (default) = the extend kernel is probed per scene (timed, remembered in the scene; pt_stats.reserved[0]
                               tells which one ran); 1 / 2 / 3 = every frame uses the one-ray-per-lane / lane-packing / pooled kernel, so
                               that runs are reproducible in speed as well as in pixels. A PT_FLAG_EXTEND_* of a frame overrides it */
    uint32_t readback;      /* how a launch's queue sizes reach the host: 0 (default) = the next launch's first thread per shard stores them
                               to host-mapped pinned memory; 1 = a 2-4 KB device-to-host copy behind every launch (a copy dispatch
                               that sits in order between two launches: rounds 1-2) */
} pt_tuning; /* 40 B */

/* ---- context: replaces GraphicsDevice.Init (GraphicsDevice.cs:38-43) + Renderer.CreateResources (Renderer.cs:105-196) */
pt_status pt_context_create(const pt_device_desc *desc, pt_context **out);
void pt_context_destroy(pt_context *ctx);                 /* Renderer.Dispose, Renderer.cs:1192-1216 */
const char *pt_last_error(const pt_context *ctx);         /* ctx may be NULL: last error of the calling thread */
pt_status pt_context_get_tuning(const pt_context *ctx, pt_tuning *out);
pt_status pt_context_set_tuning(pt_context *ctx, const pt_tuning *tuning);
uint32_t pt_abi_version(void);

/* ---- scene: the reference has only shader literals (Test.hlsl:6,8,12,13); this is the API that replaces them */
pt_status pt_scene_create(pt_context *ctx, pt_scene **out);
void pt_scene_destroy(pt_scene *scene);
/* Domain (docs/SPEC.md §4): any finite vertex is accepted; hits are the geometric ones for coordinates and hit distances within 2^±30. */
pt_status pt_scene_set_triangles(pt_scene *s, const float *verts9, const uint32_t *material_ids, uint64_t count);
/* Domain (docs/SPEC.md §4): a sphere's outline is uncertain by 7.78 (|oc|/r)^2 2^-24 of r^2: 1 % at 147 radii from the ray origin, noise at 3000. */
pt_status pt_scene_set_spheres(pt_scene *s, const float *cxyzr, const uint32_t *material_ids, uint64_t count);
pt_status pt_scene_set_materials(pt_scene *s, const pt_material *mats, uint64_t count);
pt_status pt_scene_set_camera(pt_scene *s, const pt_camera *cam);
pt_status pt_scene_set_sky(pt_scene *s, const float rgb[3]);
/* Environment map (docs/SPEC.md §11): n x n texels, row-major, 3 floats each (linear RGB radiance), octahedral layout. rgb == NULL &&
 * n == 0 removes it. 1 <= n <= 2048 and every component finite and >= 0, else PT_ERR_INVALID_ARGUMENT (a refused call keeps the previous
 * environment). While set it replaces `sky` on every miss of a PT_PATH_TRACE frame (`sky` is kept and returns when the environment is
 * removed), and PT_FLAG_NEXT_EVENT frames sample it as a light with MIS if its total is positive. Works before and after pt_scene_commit —
 * like pt_scene_set_sky it takes effect for the next pt_render without a new commit (the upload waits on the context's stream), and it
 * survives commits and geometry updates — and on a detached scene (host table only). A caller that changes it restarts accumulation.
 * Frames of a scene with an environment run on the one-ray-per-lane kernel (pt_stats.reserved[0] = 1, no kernel probe): with
 * PT_FLAG_EXTEND_PACKED / _POOL, PT_FLAG_SPLIT_KERNELS / _BUCKET_SPECULAR, PT_FLAG_COUNT_VISITS or pt_tuning.extend_kernel 2 / 3 they are
 * PT_ERR_UNSUPPORTED. PT_REFERENCE_SPHERE, pt_trace_rays, the guides of pt_denoise / pt_denoise_temporal and pt_display do not see it. */
pt_status pt_scene_set_environment(pt_scene *s, const float *rgb, uint32_t n);
typedef struct pt_environment_info { uint32_t n, lit; uint64_t device_bytes; double total; } pt_environment_info;   /* n == 0: none set; lit: 1 if it is a light for NEE */
pt_status pt_scene_environment_info(const pt_scene *s, pt_environment_info *out);
/* the sampling table exactly as the kernels read it: n*n float4 (r,g,b,p), n marginal cdf entries, n*n conditional cdf entries;
 * n_texels = the texels the three arrays have room for (>= n*n) */
pt_status pt_scene_environment_read(const pt_scene *s, float *texels4, float *mcdf, float *ccdf, uint64_t n_texels);
/* Thin-lens camera (docs/SPEC.md §3.1): depth of field. With radius > 0 every camera ray of a PT_PATH_TRACE frame starts at a point drawn
 * uniformly on the disc of that radius around the camera's origin, in the plane of `right` and `up`, and passes through the point the
 * pinhole ray of the same sample reaches at origin + focus_distance * (forward + sx * right + sy * up): what lies there is sharp, everything
 * else is blurred by a disc that grows with the aperture. radius == 0 is no lens: every frame is then bit for bit the pinhole frame. The
 * two random numbers of the disc are RNG dimensions 2 and 3, which nothing else draws, so every other random number of a path is the
 * pinhole frame's; rays and paths are counted as before.
 * Domain (docs/SPEC.md §3.1 has the rule): the ray's direction is normalize(focus_distance * v - a), a on the aperture, whose squared length
 * must be a normal, finite f32. pt_render of a frame with radius > 0 is PT_ERR_INVALID_ARGUMENT — before it replaces anything: the previous
 * frame, its sums and what was made from them stay — unless, for the frame's camera and image size, right and up span a plane
 * (|cross(right, up)| > 2^-6 |right| |up|), hi = focus_distance * max|v| + radius * sqrt(1 + |cos(right, up)|) has hi^2 <= 2^127 (max |v|
 * over the image's corners), and focus_distance * (the part of forward off that plane - 2^-11 S) >= 2^-60, S being the sum of the sizes of
 * the terms v is made from (|forward| + max|sx| |right| + max|sy| |up|, as §3.1 pads them). pt_scene_set_lens itself does
 * not apply the rule: the camera may change later. */
typedef struct pt_lens {
    float radius;          /* aperture radius in world units; finite, >= 0; 0 = pinhole */
    float focus_distance;  /* F, in units of |forward| along the view axis; finite, > 0 */
    uint32_t flags;        /* 0; any bit set is PT_ERR_INVALID_ARGUMENT */
    uint32_t pad[5];
} pt_lens;                 /* 32 B */
/* lens == NULL removes the lens. A refused call (PT_ERR_INVALID_ARGUMENT: a negative, NaN or infinite radius, a focus_distance that is not
 * finite and > 0, a flag bit) keeps the previous lens. Works before and after pt_scene_commit — like pt_scene_set_sky it takes effect with
 * the next pt_render without a new commit —, survives commits, pt_scene_update_triangles / pt_scene_update_spheres and pt_scene_set_camera
 * (the aperture follows the camera's current right and up), and works on a detached scene (host values only). A caller that changes the
 * lens restarts accumulation: the library does not notice that PT_FLAG_ACCUMULATE sums were made through another lens.
 * Frames with radius > 0 run on the one-ray-per-lane kernel with all-kinds shading (pt_stats.reserved[0] = 1, no kernel probe), with and
 * without PT_FLAG_NEXT_EVENT and an environment map: with PT_FLAG_EXTEND_PACKED / _POOL, PT_FLAG_SPLIT_KERNELS / _BUCKET_SPECULAR,
 * PT_FLAG_COUNT_VISITS or pt_tuning.extend_kernel 2 / 3 they are PT_ERR_UNSUPPORTED. They resolve no sky pixels (pt_stats.reserved[3] = 0).
 * A camera whose right or up has length 0, or whose aperture axes (radius * right / |right|, radius * up / |up|, in f32) are not finite,
 * makes such a pt_render PT_ERR_INVALID_ARGUMENT. Only PT_PATH_TRACE frames see the lens: PT_REFERENCE_SPHERE, pt_trace_rays, pt_gather,
 * the guide pass of pt_denoise / pt_denoise_temporal (with its reprojection: they keep the pinhole centre ray) and pt_display do not. */
pt_status pt_scene_set_lens(pt_scene *s, const pt_lens *lens);
pt_status pt_scene_get_lens(const pt_scene *s, pt_lens *out);   /* radius 0, focus_distance 0 when none is set */
/* Albedo textures (docs/SPEC.md §13). A scene is TEXTURED when, after pt_scene_commit, it has per-triangle UVs and at least one material
 * bound to a texture that is set; at a triangle hit of a bound material a PT_PATH_TRACE frame then reads albedo * texel (per component)
 * wherever it read the albedo: the Lambert weight, the metal and dielectric tint, the T * albedo of a light sample. Emission is not textured,
 * and a sphere keeps its material's plain albedo. A scene that is not textured renders every frame, gather, guide and blob bit for bit as
 * without these calls. The three setters behave like pt_scene_set_triangles / _materials: they work on detached scenes, mark the scene
 * uncommitted and take effect with the next pt_scene_commit, and a refused call keeps what was there. pt_scene_update_triangles keeps the
 * UVs (they belong to the triangle index). The guide pass of pt_denoise / pt_denoise_temporal writes albedo * texel into g1.rgb.
 * Textured frames run on the one-ray-per-lane kernel with all-kinds shading (pt_stats.reserved[0] = 1, no kernel probe), with and without
 * PT_FLAG_NEXT_EVENT and an environment map. PT_ERR_UNSUPPORTED on a textured scene: PT_FLAG_EXTEND_PACKED / _POOL, PT_FLAG_SPLIT_KERNELS /
 * _BUCKET_SPECULAR, PT_FLAG_COUNT_VISITS, pt_tuning.extend_kernel 2 / 3, a lens of radius > 0, PT_FLAG_NEXT_EVENT_SPHERES on a scene that has
 * a sphere light, and pt_gather_paths. pt_gather, pt_trace_rays and PT_REFERENCE_SPHERE do not look at textures.
 * Not there: textured spheres, emission or roughness maps, mip-mapping, textures under a lens or with sphere lights, textured path gathers. */
#define PT_MAX_TEXTURES 64u
#define PT_NO_TEXTURE 0xFFFFFFFFu
enum { PT_TEXTURE_NEAREST = 1u };   /* pt_scene_set_texture flags: the nearest texel instead of the bilinear lookup */
/* Six floats per triangle, (s, t) at v0, v1, v2, in the order and count of pt_scene_set_triangles. uv6 == NULL && count == 0 removes them.
 * Every value finite with |x| <= 2^20, else PT_ERR_INVALID_ARGUMENT. A count that differs from the triangle count is refused by
 * pt_scene_commit (the two setters may come in either order). Wrap is repeat. */
pt_status pt_scene_set_triangle_uvs(pt_scene *s, const float *uv6, uint64_t count);
/* Texture `index` < PT_MAX_TEXTURES: width x height texels, row-major (row 0 at t = 0), 3 floats each (linear RGB), 1 <= width, height <= 4096,
 * every component finite and >= 0. flags: 0 = bilinear, PT_TEXTURE_NEAREST; any other bit is refused. rgb == NULL with width == height == 0
 * removes the index. */
pt_status pt_scene_set_texture(pt_scene *s, uint32_t index, const float *rgb, uint32_t width, uint32_t height, uint32_t flags);
/* One entry per material: a texture index or PT_NO_TEXTURE. NULL, 0 removes the binding. A count other than the material count, or an index
 * that names no texture that is set, is refused by pt_scene_commit. */
pt_status pt_scene_set_material_textures(pt_scene *s, const uint32_t *texture_of_material, uint64_t count);
typedef struct pt_texture_info { uint32_t width, height, flags, materials; uint64_t device_bytes; } pt_texture_info; /* width 0: the index is not set; materials: how many are bound to it; device_bytes: of its texels on the device (0 on a detached scene or before a commit) */
pt_status pt_scene_texture_info(const pt_scene *s, uint32_t index, pt_texture_info *out);
/* builds the BVH on the host (binned SAH) and uploads everything; replaces CreateComputePipeline's one-time
 * descriptor/pipeline set-up (Renderer.cs:293-403). bvh_width: PT_BVH_WIDTH_* */
pt_status pt_scene_commit(pt_scene *s, uint32_t bvh_width);
pt_status pt_scene_bvh_info(const pt_scene *s, pt_bvh_info *out);
/* copies out the acceleration-structure blob (docs/SPEC.md §4.1) so that a checker can traverse the same bytes */
pt_status pt_scene_bvh_read(const pt_scene *s, void *nodes, uint64_t node_bytes, void *tris48, uint64_t tri_bytes);

/* ---- frame: replaces Renderer.ComputeFrame (Renderer.cs:1006-1040) + the fence wait (Renderer.cs:970-972) */
pt_status pt_render(pt_context *ctx, const pt_scene *scene, const pt_render_params *params, pt_stats *stats);

/* ---- ray queries (docs/SPEC.md §4.2): the closest-hit traversal of pt_render on caller rays, without a path — what a host uses
 *      for picking, visibility tests or baking. */
/* pt_trace_rays flags */
enum {
    PT_TRACE_OCCLUSION = 1u,    /* any hit with t <= tmax ends the ray (shadow / visibility query); default: closest hit */
    PT_TRACE_COUNT_VISITS = 2u, /* closest-hit only: count node visits / triangle / sphere tests into stats (slower kernel) */
    PT_TRACE_HOST_MEMORY = 4u   /* rays / hits are host pointers; the library stages them. Default: device pointers on ctx's device */
};
/* Trace n_rays caller rays against a committed scene. Synchronous on the context's stream, like pt_render.
 * rays: n_rays records of 32 B  {o.x, o.y, o.z, tmax, d.x, d.y, d.z, 0}        (f32, 16-B aligned; 4-B with PT_TRACE_HOST_MEMORY)
 * hits: n_rays records of 16 B  {t, prim_id (u32 bits), u, v}                  (f32, 16-B aligned; 4-B with PT_TRACE_HOST_MEMORY)
 * Closest hit: the smallest (t, prim_id) with t <= tmax; a miss is {+inf, 0xFFFFFFFF, 0, 0}. prim_id counts triangles 0..NT-1, then
 * spheres NT + j; (u, v) are a triangle hit's barycentrics, 0 for spheres. tmax = +inf: unbounded; tmax <= 0 or NaN: a miss. Spheres
 * need |d| = 1 (the library does not normalise); a triangle's t is in units of |d|. Device arrays must lie on ctx's device inside one
 * allocation. stats (may be NULL): rays = n_rays, gpu_ms (the query kernels, staging copies excluded), and with PT_TRACE_COUNT_VISITS
 * node_visits / tri_tests / sphere_tests. PT_TRACE_OCCLUSION | PT_TRACE_COUNT_VISITS is PT_ERR_INVALID_ARGUMENT. A query touches no
 * state of pt_render (accumulated sums, framebuffer, queues).
 * Domain (docs/SPEC.md §4): origins and hit distances within 2^±30 as for the scene; outside it the hit is specified but not the geometric one. */
pt_status pt_trace_rays(pt_context *ctx, const pt_scene *scene, const void *rays, void *hits, uint64_t n_rays,
                        uint32_t flags, pt_stats *stats);

/* ---- hemisphere gathers (docs/SPEC.md §12): ambient occlusion, sky irradiance and the bent normal at caller points — what a lightmap or
 *      probe bake wants from every texel. The K cosine-weighted rays of a point are made, traced (the occlusion query of §4.2) and summed
 *      on the device: neither a ray nor a hit record passes through memory, 32 B in and 32 B out per point whatever K is. */
enum { PT_GATHER_HOST_MEMORY = 1u };   /* points / out are host pointers, staged by the library */
typedef struct pt_gather_params {
    uint32_t samples;       /* K directions per point, 1..4096; 0 = 64 */
    uint32_t seed;
    uint32_t sample_offset; /* index of the first sample: calls over [a,b) and [b,c) merge to [a,c) */
    uint32_t point_offset;  /* added to a point's index in the RNG key: a bake split over calls or GPUs gives the same numbers */
    float max_distance;     /* occluders farther than this do not count; 0 = unbounded; else finite and > 0 */
    float ray_eps;          /* origin offset along the unit normal; finite and >= 0, taken literally */
    uint32_t flags;
    uint32_t pad;
} pt_gather_params;         /* 32 B */
/* Gather at n_points caller points of a committed scene. Synchronous on the context's stream, like pt_render.
 * points: n_points records of 32 B  {p.x, p.y, p.z, 0, n.x, n.y, n.z, 0}             (f32, 16-B aligned; 4-B with PT_GATHER_HOST_MEMORY)
 * out:    n_points records of 32 B  {E.r, E.g, E.b, visibility, bent.x, bent.y, bent.z, 0}                           (likewise)
 * Sample k of point i leaves p + ray_eps * normalize(n) in the Lambert direction d of the random numbers keyed by (seed, point_offset + i,
 * sample_offset + k); it is visible (V = 1) unless the occlusion query finds a hit within max_distance. visibility = sum V / K (the count
 * is exact: round(visibility * K) recovers it), bent = sum V d / K (unnormalised: its length is the share of unoccluded cosine-weighted
 * solid angle around its direction), E = sum V L(d) / K with L the scene's environment map if it has one, else its sky; the pdf is
 * cos / pi, so pi * E is the irradiance the sky sends to the point. The sums have one fixed order (§12): a call gives the same bits every
 * time and on every BVH layout. A point with a non-finite p or n, or with dot(n, n) zero or not finite, is invalid: it traces nothing
 * and gets {0, 0, 0, -1, 0, 0, 0, 0}. No output is ever NaN or infinite (a mean beyond the largest float is stored as that float).
 * Device arrays must lie on ctx's device inside one allocation. Checked in this order:
 *   gp NULL, unknown flag bits, samples > 4096, max_distance negative, NaN or infinite, ray_eps likewise  -> PT_ERR_INVALID_ARGUMENT
 *   ctx, scene, points or out NULL; misalignment; a detached scene or a scene of another context         -> PT_ERR_INVALID_ARGUMENT
 *   scene not committed                                                                                   -> PT_ERR_NOT_COMMITTED
 *   n_points >= 2^32                                                                                      -> PT_ERR_INVALID_ARGUMENT
 * n_points == 0 is PT_OK. stats (may be NULL): paths = n_points, rays = K * (valid points), gpu_ms (the gather kernels, staging copies
 * excluded), everything else 0. A gather touches no state of pt_render, pt_denoise* or pt_display and never runs the extend-kernel
 * probe. A failed call drains the context's stream. */
pt_status pt_gather(pt_context *ctx, const pt_scene *scene, const void *points, void *out, uint64_t n_points,
                    const pt_gather_params *gp, pt_stats *stats);

/* ---- path-traced gathers (docs/SPEC.md §12.1): what pt_gather does, with every sample a whole path of §5 that starts at the point
 *      instead of at the camera — light emitted by surfaces and light that arrives after bounces reach E, so a closed, emitter-lit
 *      scene bakes. Fused like pt_gather: 32 B in and 32 B out per point whatever samples and max_depth are. */
enum {
    PT_GATHER_PATHS_NEXT_EVENT = 4u, /* pt_gather_path_params.flags: next-event estimation in the gather (docs/SPEC.md §12.2): every sample also takes a
                                       light sample at the point itself and at each Lambert vertex of its path, combined with the hits by
                                       multiple importance sampling. (Bits 1u and 2u are unassigned and refused.) */
    PT_GATHER_PATHS_SPHERE_LIGHTS = 16u /* with PT_GATHER_PATHS_NEXT_EVENT (alone: PT_ERR_INVALID_ARGUMENT): the scene's emissive spheres join the
                                       light set, sampled by the cone they subtend (docs/SPEC.md §7.1), at the point and at every Lambert
                                       vertex. (Bit 8u is unassigned and refused.) */
};
typedef struct pt_gather_path_params {
    uint32_t max_depth;   /* path segments per sample, 1..255; 0 = 8 */
    uint32_t rr_start;    /* Russian roulette from this depth on, taken literally as in pt_render_params */
    uint32_t flags;       /* 0, PT_GATHER_PATHS_NEXT_EVENT, or that | PT_GATHER_PATHS_SPHERE_LIGHTS; any other bit is PT_ERR_INVALID_ARGUMENT */
    uint32_t pad[5];
} pt_gather_path_params;  /* 32 B */
/* points, out, n_points, gp (every field, PT_GATHER_HOST_MEMORY included), alignment and point_offset are pt_gather's. Sample k of point
 * i leaves the same origin in the same direction d as pt_gather's (same key, dimensions 0 and 1); from there §5's loop runs unchanged
 * with T = 1, depth 0, the stated max_depth and rr_start and ray_eps = gp->ray_eps, its vertices drawing dimensions 4 + 4b .. 7 + 4b of
 * that key. The point stands where the camera stands: it is no vertex and has no albedo. E = (sum of the paths' radiance) / K, summed in
 * §12's order with one fma per emission or miss term; pi * E is the irradiance for a Lambert texel. visibility and bent are pt_gather's,
 * bit for bit, for the same gp: V = 1 unless the first segment's closest hit lies within max_distance (the path itself goes on from the
 * closest hit whatever max_distance is). With max_depth 1, max_distance 0 and no emissive material the whole record is pt_gather's.
 * Invalid points, finiteness and the clamp of E are pt_gather's.
 * PT_GATHER_PATHS_NEXT_EVENT (docs/SPEC.md §12.2): the lights are the committed scene's emissive triangles (PT_FLAG_NEXT_EVENT's light set)
 * and its environment map if that is lit. Every sample takes one light sample at the point, a Lambert receiver with n = the point's
 * normal and no albedo, before its first segment, and one at every Lambert vertex of its path as a PT_FLAG_NEXT_EVENT frame does; hits of
 * lights and misses into a lit map are weighted by the power heuristic, the first segment's included. With max_depth 1 that is a
 * direct-light bake. visibility and bent do not change (shadow rays never count for them and ignore max_distance); on a scene without
 * a light of either kind the flagged call is the unflagged call bit for bit. rays then also counts the shadow rays traced.
 * PT_GATHER_PATHS_SPHERE_LIGHTS (docs/SPEC.md §7.1) adds the committed scene's emissive spheres to that light set: a light sample that picks
 * one draws a direction in the cone it subtends, and hits of such a sphere are weighted like hits of light triangles. On a scene without
 * an emissive sphere the call is the PT_GATHER_PATHS_NEXT_EVENT call bit for bit.
 * Checked first: pp NULL, a bit of pp->flags other than these two, PT_GATHER_PATHS_SPHERE_LIGHTS without PT_GATHER_PATHS_NEXT_EVENT,
 * max_depth > 255 -> PT_ERR_INVALID_ARGUMENT; then every check of pt_gather in its order.
 * n_points == 0 is PT_OK. stats (may be NULL): paths = n_points, rays = path segments (+ shadow rays) traced (exact), gpu_ms, everything
 * else 0. Touches no state of pt_render, pt_denoise*, pt_display or pt_gather, never runs the extend-kernel probe; a failed call drains
 * the context's stream.
 * Not there: next-event estimation at metal or dielectric vertices, the lens, a transmitting or glossy point. */
pt_status pt_gather_paths(pt_context *ctx, const pt_scene *scene, const void *points, void *out, uint64_t n_points,
                          const pt_gather_params *gp, const pt_gather_path_params *pp, pt_stats *stats);

/* ---- geometry updates (docs/SPEC.md §4.3): move a committed scene's triangles or spheres without a new commit — what a host's
 *      per-frame Update hook (Renderer.Update, Renderer.cs:86-89) uses to animate. The BVH keeps its topology and leaf assignment;
 *      the triangle records and every box are recomputed on the GPU from the new vertices, so the scene renders and traces exactly as
 *      a fresh commit of these vertices would. Traversal speed degrades as motion stretches the old tree: pt_bvh_info.sah_cost is
 *      recomputed by every update and is the caller's signal to commit again. n_nodes, max_depth, stack_need and the layout stay;
 *      build_ms keeps describing the commit. pt_scene_bvh_read returns the refitted blob. A later pt_scene_commit builds from the
 *      updated geometry. An update leaves the context's accumulated sums alone: a PT_FLAG_ACCUMULATE frame after it continues the old
 *      sums (the mean then mixes both geometries; pt_denoise_temporal is what keeps samples under motion). Both calls are synchronous on the context's stream; a refused call leaves the scene
 *      as it was. Checked in this order: flags, committed (PT_ERR_NOT_COMMITTED), count (must equal the committed count), NULL,
 *      the values (host arrays), then detached scenes (PT_ERR_UNSUPPORTED). */
/* pt_scene_update_triangles flags */
enum {
    PT_UPDATE_HOST_MEMORY = 1u  /* verts9 is a host pointer (staged by the library); default: a device pointer on the scene's context's device */
};
/* New positions for the committed triangles: 9 floats each, same count and order as pt_scene_set_triangles; the materials stay.
 * Non-finite coordinates are PT_ERR_INVALID_ARGUMENT (a device array is checked by a reduction before anything is written). A device
 * array must lie inside one allocation on the context's device, 4-byte aligned. stats (may be NULL): gpu_ms of the update's kernels
 * (staging copies excluded), everything else 0. */
pt_status pt_scene_update_triangles(pt_scene *s, const void *verts9, uint64_t count, uint32_t flags, pt_stats *stats);
/* New centres and radii for the committed spheres (host memory, 4 floats each, same count); materials stay. Bad spheres as
 * pt_scene_set_spheres defines them are PT_ERR_INVALID_ARGUMENT. */
pt_status pt_scene_update_spheres(pt_scene *s, const float *cxyzr, uint64_t count);

/* ---- denoising (docs/SPEC.md §8): the first-hit guide buffers of the assembled frame and an edge-aware à-trous filter over it (Dammertz
 *      et al. 2010) — what turns the few-sample frames of a render-every-frame loop (App.cs:39-42) into a watchable picture, or what a host's
 *      own denoiser needs (pt_guides_read). */
/* pt_denoise_params.flags */
enum {
    PT_DENOISE_GUIDES_ONLY = 1u,  /* trace and store the guides only: no filter pass, no denoised image */
    PT_DENOISE_NO_EDGE_STOPS = 2u /* every edge-stop weight 1: the plain B3 à-trous blur (the control the guides are measured against) */
};
/* iterations: filter passes, 0 = default (4), at most 8; pass i filters with step 2^i. sigma_*: edge-stop widths of colour, normal,
 * depth and albedo; 0 = default (docs/SPEC.md §8.2 states the defaults as exact values). */
typedef struct pt_denoise_params {
    uint32_t iterations;
    float sigma_color, sigma_normal, sigma_depth, sigma_albedo;
    uint32_t flags;
    uint32_t pad[2];
} pt_denoise_params; /* 32 B */
/* Denoise the context's assembled framebuffer, with guides traced on `scene` (the scene the frame was rendered on; its camera). Synchronous
 * on the context's stream, like pt_render. Checked in this order; a refused call changes nothing:
 *   dp NULL, unknown flag bits, iterations > 8, a negative, NaN or infinite sigma; then ctx or scene NULL   -> PT_ERR_INVALID_ARGUMENT
 *   a detached scene or a scene of another context                                                          -> PT_ERR_UNSUPPORTED
 *   scene not committed                                                                                     -> PT_ERR_NOT_COMMITTED
 *   the framebuffer holds a PT_REFERENCE_SPHERE frame                                                       -> PT_ERR_UNSUPPORTED
 *   no assembled framebuffer (a PT_PATH_TRACE frame with nranks == 1, or pt_assemble_tiles / pt_comm_* on
 *   the root, makes one)                                                                                    -> PT_ERR_NOT_COMMITTED
 * It never touches the framebuffer, the accumulated sums or anything pt_framebuffer_read* return: a later PT_FLAG_ACCUMULATE frame
 * continues as if no denoise had run. The guides (W x H of the framebuffer, 8 floats per pixel: g0 = (n.xyz, t), g1 = (albedo.rgb,
 * prim id bits); a miss is (0, 0, 0, +inf), (0, 0, 0, 0xFFFFFFFF)) and the denoised image (float4 per pixel, alpha copied) stay readable
 * until the context's next pt_render or pt_assemble_tiles; then the read functions return PT_ERR_NOT_COMMITTED, as the denoised ones do
 * after a PT_DENOISE_GUIDES_ONLY call. stats (may be NULL): rays = W*H guide rays, gpu_ms all kernels, extend_ms the guide pass,
 * other_ms the filter passes, iterations = filter passes run. A failed call drains the context's stream. */
pt_status pt_denoise(pt_context *ctx, const pt_scene *scene, const pt_denoise_params *dp, pt_stats *stats);
pt_status pt_denoised_read(pt_context *ctx, float *rgba, uint64_t n_floats);               /* row-major float4, W*H*4 floats */
pt_status pt_denoised_device_ptr(pt_context *ctx, void **dptr, uint64_t *n_floats);       /* the same on the device (valid as above) */
pt_status pt_guides_read(pt_context *ctx, float *g8, uint64_t n_floats);                  /* 8 floats per pixel: g0, g1 (W*H*8 floats) */

/* ---- temporal accumulation (docs/SPEC.md §9): keep samples while the camera or the geometry moves. Each call reprojects the accumulated
 *      image of the previous call to this frame's pixels through the two cameras and the first-hit guides, rejects what no longer lies on
 *      the pixel's surface, and blends the new frame in; the unchanged §8.2 filter then runs over the accumulated image. The loop of a host
 *      that orbits a camera: pt_scene_set_camera / pt_scene_update_triangles, pt_render (1 spp, a new seed), pt_denoise_temporal. */
/* pt_temporal_params.flags */
enum {
    PT_TEMPORAL_RESET = 1u,     /* forget the history first: this call's accumulated image is the frame itself */
    PT_TEMPORAL_MATCH_IDS = 2u, /* a history tap also needs the primitive id of the pixel it is reprojected from */
    PT_TEMPORAL_MOTION = 8u     /* follow moved geometry (docs/SPEC.md §9.1): the call records the triangles and spheres it is traced on, and the
                                   next flagged call reprojects every pixel of a moved primitive from where its surface point was. (Bit 4u is
                                   unassigned and refused.) */
};
typedef struct pt_temporal_params {
    uint32_t max_history;   /* cap of a pixel's history length; the new frame weighs at least 1/max_history. 0 = default (32); at most 1048576; 1 = no history */
    float plane_tolerance;  /* tau_p: a tap's old world position may lie this far off the pixel's plane, times the distance to the old eye. 0 = default */
    float normal_min;       /* tau_n: least dot(n, n') of a tap. 0 = default; otherwise in (0, 1] */
    uint32_t flags;
    uint32_t pad[4];
} pt_temporal_params; /* 32 B */
/* One call: traces the guides of `scene` exactly as pt_denoise does, merges the assembled framebuffer with the context's history into the
 * accumulated image (float4 per pixel: accumulated rgb, the frame's alpha) and the history lengths (1 = the pixel took no history), makes
 * them, the guides and the scene's camera the new history, and — if dp is non-NULL and lacks PT_DENOISE_GUIDES_ONLY — runs the §8.2 filter
 * of pt_denoise with the accumulated image in place of the framebuffer. The filtered image is read with pt_denoised_read /
 * pt_denoised_device_ptr and the guides with pt_guides_read; without a filter pass pt_denoised_* return PT_ERR_NOT_COMMITTED. Synchronous
 * on the context's stream. Checked in this order; a refused call changes nothing (history, results, what pt_denoise made):
 *   tp NULL, unknown tp flag bits, max_history > 1048576, a negative, NaN or infinite plane_tolerance, a normal_min
 *   outside [0, 1] or NaN                                                                                     -> PT_ERR_INVALID_ARGUMENT
 *   then pt_denoise's checks of dp (when non-NULL), then pt_denoise's checks of ctx, scene and the framebuffer, same order and statuses.
 * The accumulated image and the lengths stay readable until the context's next pt_render or pt_assemble_tiles (then
 * PT_ERR_NOT_COMMITTED). The history itself lives in the context across pt_render, pt_denoise, pt_trace_rays and geometry updates; it is
 * dropped by PT_TEMPORAL_RESET, when the framebuffer's size differs from the history's, and with the context. The framebuffer, the
 * accumulated sums of PT_FLAG_ACCUMULATE and everything pt_framebuffer_read* return are never touched. Not detected (docs/SPEC.md §9): a
 * change of lighting on an unmoved surface lags by up to max_history frames; mirrors and glass reproject their own surface; misses never
 * accumulate. stats (may be NULL): rays = W*H guide rays, paths = pixels that took history, extend_ms the guide pass, shade_ms the
 * temporal pass, other_ms the filter passes, gpu_ms their sum, iterations = filter passes run. A failed call drains the context's stream
 * and leaves the history as it was.
 * PT_TEMPORAL_MOTION (docs/SPEC.md §9.1): a successful flagged call also keeps, as part of the history, the geometry it was traced on
 * (36 B per triangle, 16 B per sphere, two sets). The next flagged call on the same scene object, with no pt_scene_commit in between,
 * compares every hit primitive's device record with that snapshot; a pixel whose primitive moved (pt_scene_update_triangles /
 * pt_scene_update_spheres) carries its surface point back to the old primitive, projects that point through the history's camera and
 * tests the taps against the surface as it was, so an animated object keeps its history instead of restarting every frame. Unmoved
 * pixels are exactly the unflagged call's; so is every pixel when the snapshot is missing (first call, after an unflagged call, another
 * scene, a commit). stats->reserved[0] = hit pixels whose primitive counted as moved (0 without the flag or a usable snapshot). Still not
 * detected: lighting changes, reflections of moved objects, a sphere's rotation, topology changes. */
pt_status pt_denoise_temporal(pt_context *ctx, const pt_scene *scene, const pt_temporal_params *tp, const pt_denoise_params *dp, pt_stats *stats);
pt_status pt_temporal_read(pt_context *ctx, float *rgba, uint64_t n_floats);          /* the accumulated image, W*H*4 */
pt_status pt_temporal_device_ptr(pt_context *ctx, void **dptr, uint64_t *n_floats);   /* the same on the device (valid as above) */
pt_status pt_temporal_history_read(pt_context *ctx, float *len, uint64_t n_floats);   /* W*H history lengths l (1 = no history taken) */

/* ---- display (docs/SPEC.md §10). The reference's display pass samples the image and writes it to an sRGB swapchain
 *      (Renderer.cs:1042-1121); pt_framebuffer_read_srgb8 reproduces exactly that, 8-bit quantisation first and no tone mapping. pt_display
 *      is the path tracer's own last stage: it takes the frame, the denoised image or the accumulated image as floats, multiplies by an
 *      exposure (given, or metered from a luminance histogram and adapted from call to call), applies a tone curve and encodes each float
 *      directly to sRGB8, so the dark codes the 8-bit detour skips are all there. */
enum { PT_DISPLAY_FRAME = 0, PT_DISPLAY_DENOISED = 1, PT_DISPLAY_TEMPORAL = 2 };          /* pt_display_params.source */
enum { PT_TONE_CLAMP = 0, PT_TONE_REINHARD = 1, PT_TONE_ACES = 2 };                        /* pt_display_params.curve */
enum { PT_DISPLAY_AUTO_EXPOSURE = 1u, PT_DISPLAY_LINEAR = 2u, PT_DISPLAY_RESET_ADAPTATION = 4u }; /* pt_display_params.flags */
typedef struct pt_display_params {
    uint32_t source, curve;
    float exposure;   /* linear multiplier (with AUTO: compensation on top of the metered one); 0 = 1; else in [2^-40, 2^40] */
    float white;      /* PT_TONE_REINHARD: the value that maps to 1; 0 = 4; else in [2^-20, 2^20] */
    float key;        /* AUTO: where the log-average luminance is put; 0 = 0.18f; else in [2^-20, 2^20] */
    float adapt;      /* AUTO: share of the way from the previous call's exposure to the metered one; 0 = 1; else in (0, 1] */
    uint32_t trim_low, trim_high; /* AUTO: per mille of the metered pixels ignored at the dark / bright end; trim_low + trim_high < 1000 */
    uint32_t flags, pad;
} pt_display_params; /* 40 B */
typedef struct pt_display_info {
    float exposure;      /* E: what every pixel was multiplied by */
    float metered;       /* E_t of this call (0 without AUTO, or when nothing was metered) */
    float log_average;   /* Y_avg (0 likewise) */
    uint32_t adapted;    /* 1: an earlier call's exposure was blended in */
    uint64_t counted, used; /* N and N' of docs/SPEC.md §10: pixels of positive luminance, and those left after the trim */
} pt_display_info; /* 32 B */
/* One call: meters the source (PT_DISPLAY_AUTO_EXPOSURE only), multiplies every pixel by the exposure, applies the curve and writes one
 * R | G<<8 | B<<16 | A<<24 word per pixel — sRGB codes, or linear UNORM8 codes with PT_DISPLAY_LINEAR; alpha is always the source's
 * alpha as UNORM8. Synchronous on the context's stream. Checked in this order; a refused call changes nothing (neither the displayed
 * image nor the adaptation state):
 *   dp NULL, an unknown source / curve / flag bit, a field outside its range above or NaN, trim_low + trim_high >= 1000
 *                                                                                                             -> PT_ERR_INVALID_ARGUMENT
 *   ctx NULL                                                                                                  -> PT_ERR_INVALID_ARGUMENT
 *   the source is not there: FRAME needs what pt_framebuffer_read needs (a frame of either mode), DENOISED what pt_denoised_read needs,
 *   TEMPORAL what pt_temporal_read needs                                                                      -> PT_ERR_NOT_COMMITTED
 * The 8-bit image, the info and the histogram are results of the frame the framebuffer holds: they stay readable across pt_denoise,
 * pt_denoise_temporal and pt_trace_rays until the context's next pt_render or pt_assemble_tiles (then PT_ERR_NOT_COMMITTED). The
 * adaptation state is one f32, the last adapted exposure: it lives in the context across all calls, is read and written by AUTO calls
 * only, and is dropped by PT_DISPLAY_RESET_ADAPTATION (before the call meters; without AUTO the flag just drops it) and with the
 * context. The framebuffer, the sums, the denoised and temporal results and the temporal history are never touched. stats (may be NULL):
 * paths = W*H, extend_ms the metering kernels, other_ms the tone kernel, gpu_ms their sum, everything else 0. A failed call drains the
 * context's stream and leaves the adaptation state as it was. */
pt_status pt_display(pt_context *ctx, const pt_display_params *dp, pt_stats *stats);
pt_status pt_display_read(pt_context *ctx, uint8_t *rgba8, uint64_t n_bytes);              /* W*H*4, RGBA byte order */
pt_status pt_display_device_ptr(pt_context *ctx, void **dptr, uint64_t *n_bytes);          /* the same on the device (valid as above) */
pt_status pt_display_info_read(pt_context *ctx, pt_display_info *out);
pt_status pt_display_histogram_read(pt_context *ctx, uint32_t *bins, uint64_t n_words);   /* 512 words; all 0 without AUTO */

/* ---- results: the reference never reads its image back (it is sampled by the display pass,
 *      Renderer.cs:1042-1121); these replace that consumer. float4 linear radiance, row-major. */
pt_status pt_framebuffer_read(pt_context *ctx, float *rgba, uint64_t n_floats);
pt_status pt_framebuffer_read_rgba8(pt_context *ctx, uint8_t *rgba8, uint64_t n_bytes); /* R8G8B8A8Unorm, Renderer.cs:124 */
pt_status pt_framebuffer_device_ptr(pt_context *ctx, void **dptr, uint64_t *n_floats);   /* row-major float4 on the device */
/* What the reference's window shows: its display pass samples the R8G8B8A8Unorm image with a nearest sampler (Renderer.cs:184-185)
 * and writes it to a B8G8R8A8Srgb swapchain (SwapChain.cs:157-158), i.e. every 8-bit linear value q becomes
 * round(255 * srgb_oetf(q / 255)). No tone mapping: radiance above 1 clips, as it does in the UNORM image. RGBA order. */
pt_status pt_framebuffer_read_srgb8(pt_context *ctx, uint8_t *rgba8, uint64_t n_bytes);

/* ---- image-space partition (docs/SPEC.md §6). After pt_render with nranks > 1 the rank's tiles sit
 * tile-major in a device staging buffer; the host gathers them (RCCL via torch.distributed or
 * ncclGather) and rank 0 calls pt_assemble_tiles on the gathered buffer. */
typedef struct {
    uint32_t tile_size, tiles_x, tiles_y, n_tiles;
    uint32_t tiles_mine;      /* tiles owned by params.rank */
    uint32_t tiles_per_rank;  /* max over ranks = stride of one rank's block in the gathered buffer, in tiles */
    uint64_t floats_per_tile; /* tile_size^2 * 4 */
} pt_tile_layout;
pt_status pt_tile_layout_query(const pt_render_params *params, pt_tile_layout *out);
/* tiles_per_rank*floats_per_tile floats. Ownership: the buffer is rewritten by the context's next pt_render, on the context's
 * own streams — a caller that hands it to an asynchronous collective on another stream must wait for that collective before it
 * renders again (bench.py does; pt_comm orders the two on one stream). */
pt_status pt_tiles_device_ptr(pt_context *ctx, void **dptr, uint64_t *n_floats);
/* gathered = nranks blocks of tiles_per_rank*floats_per_tile floats (device pointer on ctx's device) */
pt_status pt_assemble_tiles(pt_context *ctx, const pt_render_params *params, const void *gathered_dptr, uint64_t n_floats);

/* ---- several GPUs of one node behind one call (docs/SPEC.md §6). The reference is single-device (GraphicsDevice.cs:176-183) and its
 * host is one process (Program.cs:3-7), so a C# caller cannot use a process-per-GPU launcher: a pt_comm holds one pt_context per
 * rank inside the calling process. Ranks on distinct devices exchange their tiles with ONE ncclGather per frame over an RCCL
 * communicator made by ncclCommInitAll (librccl.so.1 is loaded on first use; libptrt does not link it). Ranks that share one
 * context ("virtual ranks": rehearsal of the partition on a single GPU) are rendered one after the other and staged by device
 * copies. A rank's tile buffer (pt_tiles_device_ptr) belongs to the library between pt_render and the end of the exchange. */
typedef struct pt_comm pt_comm;
enum {
    PT_COMM_FORCE_RCCL = 1u,    /* pt_comm_create flags: use the RCCL path even for a single rank (plumbing check on one GPU) */
    PT_COMM_COPY_EXCHANGE = 2u  /* no RCCL: every rank's tile block reaches the root by a device copy on the rank's own stream (a peer copy over
                                   xGMI between devices). Also lifts the one-context-per-device rule: N contexts on ONE device render
                                   concurrently, one host thread each — the multi-context code path as far as a single GPU can take it */
};
/* ctxs[i] renders rank i of n_ranks; the assembled frame lands in ctxs[root] (pt_framebuffer_read*). Either every rank has its own
 * context on its own device, or all ranks share one context, or (PT_COMM_COPY_EXCHANGE) every rank has its own context anywhere. */
pt_status pt_comm_create(pt_context *const *ctxs, uint32_t n_ranks, uint32_t root, uint32_t flags, pt_comm **out);
void pt_comm_destroy(pt_comm *comm); /* before or after its contexts: every pt_comm call returns with nothing in flight */
/* One frame: rank i renders its tiles of `params` (rank / nranks are filled in) on scenes[i] — the same scene committed on every
 * context — concurrently (one host thread per context), then the tiles are gathered to the root and assembled there.
 * stats: n_ranks entries or NULL. Synchronous, like pt_render. */
pt_status pt_comm_render(pt_comm *comm, const pt_scene *const *scenes, const pt_render_params *params, pt_stats *stats);
/* The two halves of the exchange for callers that drive pt_render themselves (rank = the rank just rendered on its context):
 * pt_comm_stage_tiles copies that rank's tile block to where the exchange wants it; pt_comm_assemble runs the exchange (if any
 * rank lives on another device) and un-tiles the gathered blocks into the root's framebuffer. */
pt_status pt_comm_stage_tiles(pt_comm *comm, uint32_t rank);
pt_status pt_comm_assemble(pt_comm *comm, const pt_render_params *params);

/* ---- deterministic synthetic scenes (C1..C5); host only, no device needed.
 * Two-call pattern: pass NULL arrays to get counts, then buffers of those sizes. */
enum {
    PT_SCENE_CORNELL = 0,        /* C1/C2: 5 walls (10 tris) + emissive ceiling quad (2 tris) + 4 Lambert spheres */
    PT_SCENE_CORNELL_GLASS = 1,  /* C4: same box, spheres = dielectric, metal (rough), 2 Lambert */
    PT_SCENE_TRIANGLE_SOUP = 2,  /* C3: `detail` random triangles in [-1,1]^3, sky emitter */
    PT_SCENE_CORNELL_TESS = 3    /* C5: Cornell with walls tessellated to ~`detail` triangles */
};
typedef struct { uint64_t n_tris, n_spheres, n_mats; } pt_scene_counts;
pt_status pt_scenegen(uint32_t kind, uint32_t detail, uint32_t seed, uint32_t width, uint32_t height,
                      pt_scene_counts *counts, float *verts9, uint32_t *tri_mat, float *spheres, uint32_t *sph_mat,
                      pt_material *mats, pt_camera *cam, float sky[3]);

#ifdef __cplusplus
}
#endif
#endif
