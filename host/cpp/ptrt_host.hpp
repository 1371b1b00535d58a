// C++ host above the C ABI (include/ptrt.h), mirroring the reference's App / Renderer shape
// (RayTracing/App.cs:7-68, RayTracing/Graphics/Renderer.cs:59-89, 933-1004, 1006-1040): throw-on-failure,
// RAII instead of IDisposable, synchronous Render(). Header-only; links against libptrt.so.
#pragma once
#include "../../include/ptrt.h"
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

namespace ptrt_host {

struct Error : std::runtime_error { pt_status status; Error(pt_status s, const std::string &m) : std::runtime_error(m), status(s) {} };
inline void check(pt_status s, const pt_context *c = nullptr)
{
    if (s != PT_OK) throw Error(s, std::string("ptrt status ") + std::to_string(s) + ": " + pt_last_error(c));
}

class Renderer {
public:
    pt_render_params Params{};
    pt_stats LastStats{};

    Renderer(uint32_t width = 1920, uint32_t height = 1080) // App.cs:27
    {
        Params.width = width; Params.height = height; Params.spp = 1; Params.max_depth = 8; Params.rr_start = 3;
        Params.seed = 0x5EED0001u; Params.mode = PT_REFERENCE_SPHERE; Params.ray_eps = 1e-4f; Params.nranks = 1; Params.streams = 8;
    }
    Renderer(const Renderer &) = delete;
    ~Renderer() { Dispose(); }

    void Init(int device = 0) // Renderer.Init, Renderer.cs:66-84
    {
        if (pt_abi_version() != PTRT_ABI_VERSION) // the library found at run time is not the one this header describes
            throw Error(PT_ERR_UNSUPPORTED, "libptrt has ABI version " + std::to_string(pt_abi_version()) + ", built against " + std::to_string(PTRT_ABI_VERSION));
        pt_device_desc d{}; d.device_ordinal = device;
        check(pt_context_create(&d, &ctx_));
    }
    void LoadSyntheticScene(uint32_t kind, uint32_t detail = 0, uint32_t seed = 0x5EED0001u, uint32_t bvh_width = 0)
    {
        pt_scene_counts n{}; pt_camera cam{}; float sky[3];
        check(pt_scenegen(kind, detail, seed, Params.width, Params.height, &n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
        std::vector<float> verts(n.n_tris * 9 + 1), sph(n.n_spheres * 4 + 1);
        std::vector<uint32_t> tm(n.n_tris + 1), sm(n.n_spheres + 1);
        std::vector<pt_material> mats(n.n_mats + 1);
        check(pt_scenegen(kind, detail, seed, Params.width, Params.height, &n, verts.data(), tm.data(), sph.data(), sm.data(), mats.data(), &cam, sky));
        if (scene_) { pt_scene_destroy(scene_); scene_ = nullptr; }
        check(pt_scene_create(ctx_, &scene_), ctx_);
        check(pt_scene_set_triangles(scene_, verts.data(), tm.data(), n.n_tris), ctx_);
        check(pt_scene_set_spheres(scene_, sph.data(), sm.data(), n.n_spheres), ctx_);
        check(pt_scene_set_materials(scene_, mats.data(), n.n_mats), ctx_);
        check(pt_scene_set_camera(scene_, &cam), ctx_);
        check(pt_scene_set_sky(scene_, sky), ctx_);
        check(pt_scene_commit(scene_, bvh_width), ctx_);
        Params.mode = PT_PATH_TRACE;
    }
    void Update(float) {}                               // Renderer.cs:86-89: empty
    void Render(float delta) { ComputeFrame(delta); }   // Renderer.cs:933-1004 without acquire/draw/present
    std::vector<float> ReadFramebuffer()
    {
        std::vector<float> px((size_t)Params.width * Params.height * 4);
        check(pt_framebuffer_read(ctx_, px.data(), px.size()), ctx_);
        return px;
    }
    std::vector<uint8_t> ReadFramebufferRgba8()
    {
        std::vector<uint8_t> px((size_t)Params.width * Params.height * 4);
        check(pt_framebuffer_read_rgba8(ctx_, px.data(), px.size()), ctx_);
        return px;
    }
    // docs/SPEC.md §8: guides on the current scene, then the edge-aware à-trous filter over the last frame (iterations 0 = default)
    pt_stats Denoise(uint32_t iterations = 0, uint32_t flags = 0)
    {
        pt_denoise_params dp{}; dp.iterations = iterations; dp.flags = flags;
        pt_stats st{};
        check(pt_denoise(ctx_, scene_, &dp, &st), ctx_);
        return st;
    }
    std::vector<float> ReadDenoised()
    {
        std::vector<float> px((size_t)Params.width * Params.height * 4);
        check(pt_denoised_read(ctx_, px.data(), px.size()), ctx_);
        return px;
    }
    // docs/SPEC.md §12: ambient occlusion, sky irradiance and the bent normal at surface points of the current scene. points: 8 floats per
    // point {p.xyz, 0, n.xyz, 0}; returns 8 floats per point {E.rgb, visibility, bent.xyz, 0}. gp.flags is set for host arrays here.
    std::vector<float> Gather(const std::vector<float> &points, pt_gather_params gp = {}, pt_stats *stats = nullptr)
    {
        if (points.size() % 8) throw Error(PT_ERR_INVALID_ARGUMENT, "Gather: 8 floats per point");
        std::vector<float> rows(points.size());
        if (points.empty()) return rows; // (an empty vector has no storage to point at)
        gp.flags |= PT_GATHER_HOST_MEMORY;
        check(pt_gather(ctx_, scene_, points.data(), rows.data(), points.size() / 8, &gp, stats), ctx_);
        return rows;
    }
    // docs/SPEC.md §12.1: Gather with every sample a whole path that starts at the point (pp.max_depth segments at most, 0 = 8; Russian
    // roulette from pp.rr_start on): E carries emission and bounced light, visibility and bent are Gather's. stats->rays: segments traced.
    std::vector<float> GatherPaths(const std::vector<float> &points, pt_gather_params gp = {}, pt_gather_path_params pp = {}, pt_stats *stats = nullptr)
    {
        if (points.size() % 8) throw Error(PT_ERR_INVALID_ARGUMENT, "GatherPaths: 8 floats per point");
        std::vector<float> rows(points.size());
        if (points.empty()) return rows; // (an empty vector has no storage to point at)
        gp.flags |= PT_GATHER_HOST_MEMORY;
        check(pt_gather_paths(ctx_, scene_, points.data(), rows.data(), points.size() / 8, &gp, &pp, stats), ctx_);
        return rows;
    }
    void SetCamera(const pt_camera &cam) { check(pt_scene_set_camera(scene_, &cam), ctx_); } // no new commit needed
    // docs/SPEC.md §11: n x n texels of linear RGB, octahedral layout; an empty vector with n = 0 removes the map. No new commit needed.
    void set_environment(const std::vector<float> &rgb, uint32_t n)
    {
        if (n && rgb.size() < (size_t)n * n * 3) throw Error(PT_ERR_INVALID_ARGUMENT, "set_environment: fewer than n * n * 3 floats");
        check(pt_scene_set_environment(scene_, n ? rgb.data() : nullptr, n), ctx_);
    }
    // docs/SPEC.md §3.1: a thin lens of aperture `radius` focused at `focus_distance` (depth of field); radius 0 is the pinhole. No new
    // commit needed; a caller that changes the lens restarts accumulation.
    void set_lens(float radius, float focus_distance)
    {
        pt_lens lens{}; lens.radius = radius; lens.focus_distance = focus_distance;
        check(pt_scene_set_lens(scene_, &lens), ctx_);
    }
    void clear_lens() { check(pt_scene_set_lens(scene_, nullptr), ctx_); }
    pt_lens lens() const { pt_lens l{}; check(pt_scene_get_lens(scene_, &l), ctx_); return l; }
    // docs/SPEC.md §13, albedo textures: per-triangle UVs (6 floats per triangle, empty = none), texture `index` (width x height texels of
    // linear RGB; an empty vector removes it) and one texture index or PT_NO_TEXTURE per material (empty = no binding). All three take
    // effect with the next commit(). Not there: textured spheres, emission or roughness maps, mip-mapping, textures under a lens or with
    // sphere lights, textured path gathers.
    void set_triangle_uvs(const std::vector<float> &uv6) { check(pt_scene_set_triangle_uvs(scene_, uv6.empty() ? nullptr : uv6.data(), uv6.size() / 6), ctx_); }
    void set_texture(uint32_t index, const std::vector<float> &rgb, uint32_t width, uint32_t height, uint32_t flags = 0)
    {
        if (rgb.size() < (size_t)width * height * 3) throw Error(PT_ERR_INVALID_ARGUMENT, "set_texture: fewer than width * height * 3 floats");
        check(pt_scene_set_texture(scene_, index, rgb.empty() ? nullptr : rgb.data(), width, height, flags), ctx_);
    }
    void set_material_textures(const std::vector<uint32_t> &texture_of_material)
    {
        check(pt_scene_set_material_textures(scene_, texture_of_material.empty() ? nullptr : texture_of_material.data(), texture_of_material.size()), ctx_);
    }
    pt_texture_info texture_info(uint32_t index) const { pt_texture_info i{}; check(pt_scene_texture_info(scene_, index, &i), ctx_); return i; }
    void commit(uint32_t bvh_width = 0) { check(pt_scene_commit(scene_, bvh_width), ctx_); }
    // docs/SPEC.md §9: reproject the previous call's accumulated image to this frame and blend the last frame in; with `filter` the
    // §8.2 filter then runs over the result (ReadDenoised). Zeros mean the defaults; the context keeps the history between calls.
    pt_stats DenoiseTemporal(uint32_t max_history = 0, uint32_t flags = 0, bool filter = true, uint32_t iterations = 0)
    {
        pt_temporal_params tp{}; tp.max_history = max_history; tp.flags = flags;
        pt_denoise_params dp{}; dp.iterations = iterations;
        pt_stats st{};
        check(pt_denoise_temporal(ctx_, scene_, &tp, filter ? &dp : nullptr, &st), ctx_);
        return st;
    }
    std::vector<float> ReadTemporal()
    {
        std::vector<float> px((size_t)Params.width * Params.height * 4);
        check(pt_temporal_read(ctx_, px.data(), px.size()), ctx_);
        return px;
    }
    std::vector<float> ReadHistoryLength()
    {
        std::vector<float> len((size_t)Params.width * Params.height);
        check(pt_temporal_history_read(ctx_, len.data(), len.size()), ctx_);
        return len;
    }
    // The display stage (include/ptrt.h pt_display, docs/SPEC.md §10), where the reference's display pass samples the image
    // (Renderer.cs:1042-1121): source PT_DISPLAY_*, curve PT_TONE_*, flags PT_DISPLAY_*; the other fields of dp keep their defaults
    pt_stats Display(uint32_t source = PT_DISPLAY_FRAME, uint32_t curve = PT_TONE_CLAMP, uint32_t flags = 0, float exposure = 0.0f)
    {
        pt_display_params dp{}; dp.source = source; dp.curve = curve; dp.flags = flags; dp.exposure = exposure;
        return Display(dp);
    }
    pt_stats Display(const pt_display_params &dp)
    {
        pt_stats st{};
        check(pt_display(ctx_, &dp, &st), ctx_);
        return st;
    }
    std::vector<uint8_t> ReadDisplay()
    {
        std::vector<uint8_t> px((size_t)Params.width * Params.height * 4);
        check(pt_display_read(ctx_, px.data(), px.size()), ctx_);
        return px;
    }
    pt_display_info DisplayInfo()
    {
        pt_display_info info{};
        check(pt_display_info_read(ctx_, &info), ctx_);
        return info;
    }
    std::vector<uint32_t> ReadDisplayHistogram()
    {
        std::vector<uint32_t> bins(512);
        check(pt_display_histogram_read(ctx_, bins.data(), bins.size()), ctx_);
        return bins;
    }
    void Dispose()
    {
        if (scene_) pt_scene_destroy(scene_);
        if (ctx_) pt_context_destroy(ctx_);
        scene_ = nullptr; ctx_ = nullptr;
    }
    pt_context *Context() const { return ctx_; }
    pt_scene *Scene() const { return scene_; }

private:
    void ComputeFrame(float) // Renderer.cs:1006-1040 + fence wait :972
    {
        check(pt_render(ctx_, Params.mode == PT_PATH_TRACE ? scene_ : nullptr, &Params, &LastStats), ctx_);
    }
    pt_context *ctx_ = nullptr;
    pt_scene *scene_ = nullptr;
};

// One frame over several GPUs of the node (include/ptrt.h pt_comm): a Renderer per device, the same scene committed on each, tiles
// dealt round-robin, one ncclGather per frame inside libptrt. `virtual_ranks`: every rank on device 0 through one Renderer
// (rehearsal on a single GPU). The reference is single-device; this is what stands above its Renderer when a node has 8 GPUs.
class MultiRenderer {
public:
    pt_render_params Params{};
    std::vector<pt_stats> LastStats;

    // mode 0: one device per rank, one RCCL gather per frame; 1: virtual ranks (one context renders the ranks one after the other);
    // 2: one context per rank, all on device 0, rendered concurrently, tiles exchanged by device copies (PT_COMM_COPY_EXCHANGE)
    MultiRenderer(uint32_t n_ranks, uint32_t width, uint32_t height, int mode = 0) : n_(n_ranks), virtual_(mode == 1), one_device_(mode == 2)
    {
        const uint32_t n_ctx = virtual_ ? 1u : n_;
        for (uint32_t i = 0; i < n_ctx; ++i) r_.emplace_back(new Renderer(width, height));
        Params = r_[0]->Params;
    }
    MultiRenderer(const MultiRenderer &) = delete;
    ~MultiRenderer() { Dispose(); }
    void Init()
    {
        for (size_t i = 0; i < r_.size(); ++i) r_[i]->Init(one_device_ ? 0 : (int)i);
    }
    void LoadSyntheticScene(uint32_t kind, uint32_t detail = 0, uint32_t seed = 0x5EED0001u, uint32_t bvh_width = 0)
    {
        for (auto &r : r_) r->LoadSyntheticScene(kind, detail, seed, bvh_width); // replicated scene
        Params.mode = PT_PATH_TRACE;
        std::vector<pt_context *> ctxs(n_);
        for (uint32_t i = 0; i < n_; ++i) ctxs[i] = r_[virtual_ ? 0 : i]->Context();
        if (comm_) pt_comm_destroy(comm_);
        comm_ = nullptr;
        check(pt_comm_create(ctxs.data(), n_, 0, one_device_ ? PT_COMM_COPY_EXCHANGE : 0u, &comm_));
    }
    void Render(float)
    {
        std::vector<const pt_scene *> scenes(n_);
        for (uint32_t i = 0; i < n_; ++i) scenes[i] = r_[virtual_ ? 0 : i]->Scene();
        LastStats.assign(n_, pt_stats{});
        check(pt_comm_render(comm_, scenes.data(), &Params, LastStats.data()), r_[0]->Context());
        r_[0]->Params = Params;
    }
    void set_environment(const std::vector<float> &rgb, uint32_t n) { for (auto &r : r_) r->set_environment(rgb, n); }
    // docs/SPEC.md §13: the same UVs, texture 0 and binding on every rank's replica of the scene, committed
    void set_textured(const std::vector<float> &uv6, const std::vector<float> &rgb, uint32_t width, uint32_t height, const std::vector<uint32_t> &texture_of_material)
    {
        for (auto &r : r_) { r->set_triangle_uvs(uv6); r->set_texture(0, rgb, width, height); r->set_material_textures(texture_of_material); r->commit(); }
    }
    void set_lens(float radius, float focus_distance) { for (auto &r : r_) r->set_lens(radius, focus_distance); }
    Renderer &Root() { return *r_[0]; }
    void Dispose()
    {
        if (comm_) pt_comm_destroy(comm_);
        comm_ = nullptr;
        r_.clear();
    }

private:
    uint32_t n_;
    bool virtual_, one_device_;
    std::vector<std::unique_ptr<Renderer>> r_;
    pt_comm *comm_ = nullptr;
};

} // namespace ptrt_host
