// pipeline.h — the one statement of which pipeline a path-traced frame runs (DESIGN.md "Pipelines"): what the frame's PT_FLAG_*,
// pt_tuning.extend_kernel and the scene's environment map, lens and materials decode to, which combinations are refused, and everything the
// frame loop (frame.cpp) and the launchers (kernels.hip) derive from that. Host-only and free of HIP: tests/pipeline_ref builds it with a
// plain C++ compiler and walks every input.
#pragma once
#include <stdint.h>
#include "../../include/ptrt.h"

namespace ptrt {

// The extend kernels (pt_stats.reserved[0], pt_tuning.extend_kernel 1 / 2 / 3):
//   EXT_SIMPLE  one ray per lane;
//   EXT_PACKED  a wavefront owns `packed_chunk` (>= 64) queue entries and refills idle lanes, shading each finished ray on the spot;
//   EXT_POOL    a wavefront owns kPool entries, refills idle lanes during traversal and shades the whole pool at full width.
enum ExtendKernel : int { EXT_SIMPLE = 1, EXT_PACKED = 2, EXT_POOL = 3 };
constexpr uint32_t kExtendKernelFirst = EXT_SIMPLE, kExtendKernelLast = EXT_POOL;
// What shades a hit. As an extend kernel's `fuse`: SHADE_NONE = it only writes the hit record and k_shade follows; SHADE_QUEUE /
// SHADE_INLINE = it also shades (Lambert-only scene, lean code / all kinds) and queues the next iteration. As k_shade's mode: SHADE_QUEUE =
// queue order, specular kinds deferred to buckets; SHADE_BUCKETS = the specular buckets; SHADE_INLINE = queue order, everything in place.
enum ShadeMode { SHADE_NONE = -1, SHADE_QUEUE = 0, SHADE_BUCKETS = 1, SHADE_INLINE = 2 };
// What k_generate writes. GEN_STATE: every slot's initial path state (k_shade and k_extend_pool read it back). GEN_QUEUE: queue and
// counters only — the frame's first launch is a fused one-ray-per-lane or lane-packing kernel, which builds the state in registers.
// GEN_DENSE: like GEN_QUEUE with the queue dense (only slots that hold a path: frames in which whole sample streams are empty).
enum GenerateMode : uint32_t { GEN_QUEUE = 0, GEN_STATE = 1, GEN_DENSE = 2 };

// Which k_extend / k_extend_packed / k_extend_pool instantiations exist (each for every node layout). Next-event estimation and the
// environment map live in the one-ray-per-lane kernel only, fused and without visit counters — a shadow ray's traversal stops at its tmax,
// which the counters do not describe —, the environment with all-kinds shading whatever the materials; the pooled kernel always shades.
// The thin lens (docs/SPEC.md §3.1) lives there too, with all-kinds shading, with and without NEE and the environment: 4 instantiations.
// Sphere lights (docs/SPEC.md §7.1) are NEE's, with all-kinds shading, with and without the environment and the lens: 4 more.
// Albedo textures (docs/SPEC.md §13) live there as well, with all-kinds shading, with and without NEE and the environment, and neither through
// a lens nor with sphere lights: 4 more, not 12.
constexpr bool extend_instantiated(int kernel, int fuse, bool count, bool nee, bool env, bool lens = false, bool sph = false, bool tex = false)
{
    if (kernel < EXT_SIMPLE || kernel > EXT_POOL || fuse == SHADE_BUCKETS || fuse < SHADE_NONE || fuse > SHADE_INLINE) return false;
    if (tex) return kernel == EXT_SIMPLE && !count && fuse == SHADE_INLINE && !lens && !sph;
    if (sph) return nee && kernel == EXT_SIMPLE && !count && fuse == SHADE_INLINE;
    if (lens) return kernel == EXT_SIMPLE && !count && fuse == SHADE_INLINE;
    if (env) return kernel == EXT_SIMPLE && !count && fuse == SHADE_INLINE;
    if (nee) return kernel == EXT_SIMPLE && !count && fuse != SHADE_NONE;
    return kernel != EXT_POOL || fuse != SHADE_NONE;
}

struct Pipeline {
    uint32_t forced;        // ExtendKernel a frame flag, pt_tuning.extend_kernel, NEE, the environment, the lens or textures force (0 = none: the scene's probed choice)
    bool profile, count;    // PT_FLAG_PROFILE_KERNELS, PT_FLAG_COUNT_VISITS
    bool split, bucket;     // k_shade as a second kernel (PT_FLAG_SPLIT_KERNELS); with the specular kinds shaded from buckets (_BUCKET_SPECULAR)
    bool nee;               // PT_FLAG_NEXT_EVENT (docs/SPEC.md §7)
    bool env;               // the scene has an environment map (docs/SPEC.md §11)
    ShadeMode shade;        // Lambert-only scene: lean code; all kinds with specular materials, and with an environment, a lens or sphere lights (their instantiations shade every kind)
    bool lens;              // the scene's lens has a radius > 0 (docs/SPEC.md §3.1)
    bool sph;               // PT_FLAG_NEXT_EVENT_SPHERES on a scene that has a sphere light (docs/SPEC.md §7.1); without one the frame is the NEE frame
    bool tex;               // the scene is textured (docs/SPEC.md §13): UVs and a material bound to a texture that is set

    // One kernel per iteration by default: every extend kernel shades its own hits. The split pipelines run k_shade behind it.
    constexpr ShadeMode fuse() const { return split ? SHADE_NONE : shade; }
    // The fused one-ray-per-lane and lane-packing kernels build a slot's initial state in registers in their first launch; k_shade (split
    // pipelines) and the pooled kernel read it from memory.
    constexpr bool full_state() const { return split || forced == (uint32_t)EXT_POOL; }
    // (dense: whole sample streams have no sample, spp < streams)
    constexpr GenerateMode generate_mode(bool dense) const { return full_state() ? GEN_STATE : dense ? GEN_DENSE : GEN_QUEUE; }
    // Re-packing forced: buckets re-append (no fixed positions), or next to nothing regenerates (every launch leaves holes).
    constexpr bool forces_compact(bool repack_sticky, uint32_t samples_per_stream) const { return bucket || (repack_sticky && samples_per_stream <= 2u); }
    // Sky pixels are resolved by the frames whose first launch builds the slots' state in registers (next-event estimation included: a
    // camera ray's miss adds the sky with weight 1 there too). Not by counting frames, whose visit counters are the spec's, nor with an
    // environment map, where a miss depends on the ray's direction, nor through a lens, whose rays leave the frustum the bound is made for.
    constexpr bool resolves_sky() const { return !full_state() && !count && !env && !lens; }
    // Counting / profiling frames neither probe the extend kernel nor feed the scene's choice: their kernels are instrumented builds.
    constexpr bool instrumented() const { return count || profile; }
    // Timed kernels run alone: instrumented frames, and a frame that probes (so that its timed iterations compare), run one wavefront loop.
    constexpr bool single_loop(bool probing) const { return instrumented() || probing; }
    // The kernel of one launch. choice: the ExtendKernel the frame settled on, 0 while it probes; probe_iteration: 2 or 3 for the two timed
    // launches of a probing frame (the second runs the lane-packing kernel), else 0. The pooled kernel has no extend-only form: a split
    // frame that asks for it runs the one-ray-per-lane kernel.
    constexpr ExtendKernel kernel_for(uint32_t choice, uint32_t probe_iteration) const
    {
        return (choice == (uint32_t)EXT_PACKED || (choice == 0u && probe_iteration == 3u)) ? EXT_PACKED : (choice == (uint32_t)EXT_POOL && !split) ? EXT_POOL : EXT_SIMPLE;
    }
};

struct PipelineDecode { pt_status status; const char *message; Pipeline pipeline; }; // PT_OK: `pipeline` is filled; else refused, `message` says why

// A frame's PT_FLAG_EXTEND_* beats pt_tuning.extend_kernel (tuned_kernel), which beats the scene's own choice. An environment map and
// next-event estimation force the one-ray-per-lane kernel, the only one with their instantiations (extend_instantiated), and refuse what
// asks for another, and so does a lens: the environment first, then the lens, then NEE with another kernel, then NEE with counting.
// PT_FLAG_NEXT_EVENT_SPHERES without PT_FLAG_NEXT_EVENT is refused before all of that; with it, it refuses what NEE refuses.
// A textured scene (has_textures) forces the one-ray-per-lane kernel with all-kinds shading too and refuses, before the others speak, what
// asks for another kernel or for counting, then a lens, then sphere lights (extend_instantiated: it has neither of those forms).
constexpr PipelineDecode decode_pipeline(uint32_t flags, uint32_t tuned_kernel, bool has_env, bool has_specular, bool has_lens = false,
                                         bool has_sphere_light = false, bool has_textures = false)
{
    Pipeline p{};
    if ((flags & PT_FLAG_NEXT_EVENT_SPHERES) && !(flags & PT_FLAG_NEXT_EVENT))
        return { PT_ERR_INVALID_ARGUMENT, "PT_FLAG_NEXT_EVENT_SPHERES needs PT_FLAG_NEXT_EVENT", p };
    p.profile = (flags & PT_FLAG_PROFILE_KERNELS) != 0; p.count = (flags & PT_FLAG_COUNT_VISITS) != 0;
    p.bucket = (flags & PT_FLAG_BUCKET_SPECULAR) != 0; p.split = p.bucket || (flags & PT_FLAG_SPLIT_KERNELS) != 0;
    p.nee = (flags & PT_FLAG_NEXT_EVENT) != 0; p.env = has_env; p.lens = has_lens;
    p.sph = p.nee && (flags & PT_FLAG_NEXT_EVENT_SPHERES) != 0 && has_sphere_light;
    p.tex = has_textures;
    p.shade = (has_specular || has_env || has_lens || p.sph || p.tex) ? SHADE_INLINE : SHADE_QUEUE;
    p.forced = (flags & PT_FLAG_EXTEND_POOL) ? (uint32_t)EXT_POOL : (flags & PT_FLAG_EXTEND_PACKED) ? (uint32_t)EXT_PACKED
               : (flags & PT_FLAG_EXTEND_SIMPLE) ? (uint32_t)EXT_SIMPLE : tuned_kernel;
    const bool other_kernel = p.split || p.forced == (uint32_t)EXT_PACKED || p.forced == (uint32_t)EXT_POOL;
    if (p.tex && (other_kernel || p.count))
        return { PT_ERR_UNSUPPORTED, "a textured scene (docs/SPEC.md §13) renders on the one-ray-per-lane kernel only: not with PT_FLAG_EXTEND_PACKED, "
                                     "PT_FLAG_EXTEND_POOL, PT_FLAG_SPLIT_KERNELS, PT_FLAG_BUCKET_SPECULAR, PT_FLAG_COUNT_VISITS or pt_tuning.extend_kernel 2 / 3", p };
    if (p.tex && p.lens)
        return { PT_ERR_UNSUPPORTED, "a textured scene does not render through a lens (pt_scene_set_lens, radius > 0): remove the lens or the textures", p };
    if (p.tex && p.sph)
        return { PT_ERR_UNSUPPORTED, "a textured scene with a sphere light does not render with PT_FLAG_NEXT_EVENT_SPHERES", p };
    if (p.env && (other_kernel || p.count))
        return { PT_ERR_UNSUPPORTED, "a scene with an environment map renders on the one-ray-per-lane kernel only: not with PT_FLAG_EXTEND_PACKED, "
                                     "PT_FLAG_EXTEND_POOL, PT_FLAG_SPLIT_KERNELS, PT_FLAG_BUCKET_SPECULAR, PT_FLAG_COUNT_VISITS or pt_tuning.extend_kernel 2 / 3", p };
    if (p.lens && (other_kernel || p.count))
        return { PT_ERR_UNSUPPORTED, "a frame through a lens (pt_scene_set_lens, radius > 0) renders on the one-ray-per-lane kernel only: not with PT_FLAG_EXTEND_PACKED, "
                                     "PT_FLAG_EXTEND_POOL, PT_FLAG_SPLIT_KERNELS, PT_FLAG_BUCKET_SPECULAR, PT_FLAG_COUNT_VISITS or pt_tuning.extend_kernel 2 / 3", p };
    if (p.nee && other_kernel)
        return { PT_ERR_UNSUPPORTED, "PT_FLAG_NEXT_EVENT runs on the one-ray-per-lane kernel only: not with PT_FLAG_EXTEND_PACKED, "
                                     "PT_FLAG_EXTEND_POOL, PT_FLAG_SPLIT_KERNELS, PT_FLAG_BUCKET_SPECULAR or pt_tuning.extend_kernel 2 / 3", p };
    if (p.nee && p.count) return { PT_ERR_UNSUPPORTED, "PT_FLAG_NEXT_EVENT does not count visits (PT_FLAG_COUNT_VISITS)", p };
    if (p.env || p.nee || p.lens || p.tex) p.forced = EXT_SIMPLE;
    return { PT_OK, nullptr, p };
}

} // namespace ptrt
