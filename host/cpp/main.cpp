// ptrt_cli — headless counterpart of Program.cs / App.Run (RayTracing/Program.cs:1-9, App.cs:15-21):
// build a renderer, render N frames, write the image the reference would have shown in its window.
//   ptrt_cli [--scene reference|cornell|glass|soup|tess] [--detail N] [--size WxH] [--spp N] [--depth N]
//            [--frames N] [--ppm out.ppm] [--pfm out.pfm] [--gpus N] [--virtual 0|1|2] [--nee] [--nee-spheres] [--denoise N]
//            [--display clamp|reinhard|aces] [--auto-exposure] [--env FILE.pfm] [--texture FILE.pfm]
// --nee: next-event estimation (PT_FLAG_NEXT_EVENT, docs/SPEC.md §7). --nee-spheres: that with the scene's emissive spheres as lights
//            too (PT_FLAG_NEXT_EVENT | PT_FLAG_NEXT_EVENT_SPHERES, §7.1).
// --env FILE.pfm: a square colour PFM read as the scene's octahedral environment map (docs/SPEC.md §11; rows in file order).
// --texture FILE.pfm: a colour PFM of at most 4096 x 4096 (linear RGB, rows in file order) mapped onto the scene's Lambert surfaces that do
// not emit — the walls of the Cornell scenes — as texture 0 with planar UVs made here (docs/SPEC.md §13: every triangle projected along the
// dominant axis of its normal, one repeat per two world units).
// --denoise N: denoise the last frame with N filter passes (0 = the default; docs/SPEC.md §8) and write the denoised image to --ppm /
// --pfm instead of the frame (the PPM by SPEC §1's unorm8 rule).
// --display CURVE: run the display stage (docs/SPEC.md §10: exposure, tone curve, sRGB8 encode on the device) over the last stage that
// ran — the denoised image with --denoise, else the frame — and write its image to --ppm. --auto-exposure meters the exposure
// (alone it implies --display clamp).
// --gpus N: the frame's tiles over N devices of this node, one RCCL gather per frame (pt_comm); with --virtual 1 the N ranks are
// rendered one after the other on device 0 (rehearsal of the partition on a single GPU); with --virtual 2 every rank has its own
// context on device 0, the ranks render concurrently (one host thread each) and exchange their tiles by device copies.
#include "ptrt_host.hpp"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <utility>

// A square colour PFM ("PF", either byte order by the sign of its scale) as n x n x 3 floats, rows in file order
static std::vector<float> read_pfm(const std::string &path, uint32_t &width, uint32_t &height, bool square, unsigned limit);
static std::vector<float> read_square_pfm(const std::string &path, uint32_t &n) { uint32_t h = 0; return read_pfm(path, n, h, true, 2048); }

// A colour PFM of at most limit x limit (square: and as wide as it is high) as width x height x 3 floats, rows in file order
static std::vector<float> read_pfm(const std::string &path, uint32_t &width, uint32_t &height, bool square, unsigned limit)
{
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("cannot open " + path);
    char magic[3] = { 0, 0, 0 }; unsigned w = 0, h = 0; float scale = 0.f;
    const bool head = std::fscanf(f, "%2s %u %u %f", magic, &w, &h, &scale) == 4 && std::fgetc(f) != EOF;
    if (!head || std::strcmp(magic, "PF") != 0 || (square && w != h) || w == 0 || h == 0 || w > limit || h > limit) {
        std::fclose(f);
        throw std::runtime_error(path + (square ? ": not a square colour PFM of at most " : ": not a colour PFM of at most ") + std::to_string(limit) + " x " + std::to_string(limit));
    }
    std::vector<float> px((size_t)w * h * 3);
    const bool whole = std::fread(px.data(), sizeof(float), px.size(), f) == px.size();
    std::fclose(f);
    if (!whole) throw std::runtime_error(path + ": truncated");
    const uint16_t one = 1; const bool host_little = *(const uint8_t *)&one == 1;
    if ((scale < 0.f) != host_little)
        for (float &v : px) { uint8_t b[4]; std::memcpy(b, &v, 4); std::swap(b[0], b[3]); std::swap(b[1], b[2]); std::memcpy(&v, b, 4); }
    width = w; height = h;
    return px;
}

// docs/SPEC.md §13 for a synthetic scene: planar UVs for every triangle (projected along the dominant axis of its normal, one repeat per
// two world units, so a wall of the [-1, 1] box shows the image once) and texture 0 bound to every Lambert material that does not emit
static void planar_texturing(uint32_t kind, uint32_t detail, uint32_t w, uint32_t h, std::vector<float> &uv6, std::vector<uint32_t> &binding)
{
    pt_scene_counts n{};
    if (pt_scenegen(kind, detail, 0x5EED0001u, w, h, &n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != PT_OK) throw std::runtime_error("pt_scenegen failed");
    std::vector<float> verts(n.n_tris * 9 + 1), sph(n.n_spheres * 4 + 1);
    std::vector<uint32_t> tm(n.n_tris + 1), sm(n.n_spheres + 1);
    std::vector<pt_material> mats(n.n_mats + 1);
    pt_camera cam{}; float sky[3];
    if (pt_scenegen(kind, detail, 0x5EED0001u, w, h, &n, verts.data(), tm.data(), sph.data(), sm.data(), mats.data(), &cam, sky) != PT_OK) throw std::runtime_error("pt_scenegen failed");
    uv6.assign(n.n_tris * 6, 0.f);
    for (size_t i = 0; i < n.n_tris; ++i) {
        const float *v = &verts[i * 9];
        const float e1[3] = { v[3] - v[0], v[4] - v[1], v[5] - v[2] }, e2[3] = { v[6] - v[0], v[7] - v[1], v[8] - v[2] };
        const float nx = std::fabs(e1[1] * e2[2] - e1[2] * e2[1]), ny = std::fabs(e1[2] * e2[0] - e1[0] * e2[2]), nz = std::fabs(e1[0] * e2[1] - e1[1] * e2[0]);
        const int a = nx >= ny && nx >= nz ? 0 : ny >= nz ? 1 : 2, s = a == 0 ? 1 : 0, t = a == 2 ? 1 : 2;
        for (int k = 0; k < 3; ++k) { uv6[i * 6 + 2 * k] = v[3 * k + s] * 0.5f + 0.5f; uv6[i * 6 + 2 * k + 1] = v[3 * k + t] * 0.5f + 0.5f; }
    }
    binding.assign(n.n_mats, PT_NO_TEXTURE);
    for (size_t m = 0; m < n.n_mats; ++m)
        if (mats[m].kind == PT_LAMBERT && mats[m].emission[0] == 0.f && mats[m].emission[1] == 0.f && mats[m].emission[2] == 0.f) binding[m] = 0u;
}

int main(int argc, char **argv)
{
    std::string scene = "reference", ppm = "frame.ppm", pfm, env, texture;
    uint32_t w = 1920, h = 1080, detail = 0, spp = 64, depth = 8, frames = 1, gpus = 1, virt = 0, flags = 0;
    int denoise = -1; // filter passes of --denoise (0 = default); -1 = no denoise
    int curve = -1;   // PT_TONE_* of --display; -1 = no display stage
    bool auto_exposure = false;
    for (int i = 1; i < argc; i += 2) {
        const std::string a = argv[i];
        if (a == "--nee") { flags |= PT_FLAG_NEXT_EVENT; --i; continue; } // a switch: no value
        if (a == "--nee-spheres") { flags |= PT_FLAG_NEXT_EVENT | PT_FLAG_NEXT_EVENT_SPHERES; --i; continue; }
        if (a == "--auto-exposure") { auto_exposure = true; --i; continue; }
        if (i + 1 >= argc) { std::fprintf(stderr, "option %s needs a value\n", a.c_str()); return 2; }
        if (a == "--scene") scene = argv[i + 1];
        else if (a == "--detail") detail = (uint32_t)std::strtoul(argv[i + 1], nullptr, 0);
        else if (a == "--size") std::sscanf(argv[i + 1], "%ux%u", &w, &h);
        else if (a == "--spp") spp = (uint32_t)std::atoi(argv[i + 1]);
        else if (a == "--depth") depth = (uint32_t)std::atoi(argv[i + 1]);
        else if (a == "--frames") frames = (uint32_t)std::atoi(argv[i + 1]);
        else if (a == "--gpus") gpus = (uint32_t)std::atoi(argv[i + 1]);
        else if (a == "--virtual") virt = (uint32_t)std::atoi(argv[i + 1]);
        else if (a == "--ppm") ppm = argv[i + 1];
        else if (a == "--pfm") pfm = argv[i + 1];
        else if (a == "--env") env = argv[i + 1];
        else if (a == "--texture") texture = argv[i + 1];
        else if (a == "--denoise") denoise = std::atoi(argv[i + 1]);
        else if (a == "--display") {
            const std::string v = argv[i + 1];
            curve = v == "clamp" ? PT_TONE_CLAMP : v == "reinhard" ? PT_TONE_REINHARD : v == "aces" ? PT_TONE_ACES : -1;
            if (curve < 0) { std::fprintf(stderr, "--display takes clamp, reinhard or aces, not %s\n", v.c_str()); return 2; }
        }
        else { std::fprintf(stderr, "unknown option %s\n", a.c_str()); return 2; }
    }
    if (auto_exposure && curve < 0) curve = PT_TONE_CLAMP;
    try {
        std::unique_ptr<ptrt_host::Renderer> single;
        std::unique_ptr<ptrt_host::MultiRenderer> multi;
        const uint32_t kind = scene == "cornell" ? PT_SCENE_CORNELL : scene == "glass" ? PT_SCENE_CORNELL_GLASS
                            : scene == "soup" ? PT_SCENE_TRIANGLE_SOUP : PT_SCENE_CORNELL_TESS;
        std::vector<float> tex_rgb, tex_uv; std::vector<uint32_t> tex_binding; uint32_t tex_w = 0, tex_h = 0;
        if (!texture.empty() && scene != "reference") { tex_rgb = read_pfm(texture, tex_w, tex_h, false, 4096); planar_texturing(kind, detail, w, h, tex_uv, tex_binding); }
        if (gpus > 1 && scene != "reference") {
            multi.reset(new ptrt_host::MultiRenderer(gpus, w, h, (int)virt));
            multi->Init();
            multi->LoadSyntheticScene(kind, detail);
            if (!env.empty()) { uint32_t n = 0; const auto map = read_square_pfm(env, n); multi->set_environment(map, n); }
            if (tex_w) multi->set_textured(tex_uv, tex_rgb, tex_w, tex_h, tex_binding);
            multi->Params.spp = spp; multi->Params.max_depth = depth; multi->Params.flags |= flags;
            for (uint32_t f = 0; f < frames; ++f) multi->Render(0.f);
            unsigned long long rays = 0; double ms = 0;
            for (const pt_stats &s : multi->LastStats) { rays += s.rays; ms = s.gpu_ms > ms ? s.gpu_ms : ms; }
            std::printf("%llu rays over %u ranks, slowest rank %.3f ms\n", rays, gpus, ms);
        } else {
            single.reset(new ptrt_host::Renderer(w, h));
            single->Init();
            if (scene != "reference") {
                single->LoadSyntheticScene(kind, detail);
                if (!env.empty()) { uint32_t n = 0; const auto map = read_square_pfm(env, n); single->set_environment(map, n); }
                if (tex_w) { single->set_triangle_uvs(tex_uv); single->set_texture(0, tex_rgb, tex_w, tex_h); single->set_material_textures(tex_binding); single->commit(); }
                single->Params.spp = spp; single->Params.max_depth = depth; single->Params.flags |= flags;
            }
            for (uint32_t f = 0; f < frames; ++f) single->Render(0.f);
            const pt_stats &s = single->LastStats;
            std::printf("%llu rays, %.3f ms, %.1f Mrays/s\n", (unsigned long long)s.rays, s.gpu_ms, s.rays / s.gpu_ms / 1e3);
        }
        ptrt_host::Renderer &r = multi ? multi->Root() : *single;
        std::vector<float> denoised;
        if (denoise >= 0) {
            const pt_stats d = r.Denoise((uint32_t)denoise);
            std::printf("denoise: %u passes, guides %.3f ms, filter %.3f ms\n", d.iterations, d.extend_ms, d.other_ms);
            denoised = r.ReadDenoised();
        }
        if (!ppm.empty()) { // 8-bit image = the reference's R8G8B8A8Unorm storage image (Renderer.cs:124)
            std::vector<uint8_t> px;
            if (curve >= 0) { // the display stage's own image of the last stage that ran
                const pt_stats d = r.Display(denoise >= 0 ? PT_DISPLAY_DENOISED : PT_DISPLAY_FRAME, (uint32_t)curve,
                                             auto_exposure ? PT_DISPLAY_AUTO_EXPOSURE : 0u);
                std::printf("display: exposure %g, metering %.3f ms, tone %.3f ms\n", (double)r.DisplayInfo().exposure, d.extend_ms, d.other_ms);
                px = r.ReadDisplay();
            } else if (denoise >= 0) { // the same rule on the host: docs/SPEC.md §1 unorm8 (NaN -> 0)
                px.resize(denoised.size());
                for (size_t i = 0; i < px.size(); ++i) {
                    const float c = denoised[i];
                    px[i] = !(c > 0.0f) ? 0 : c >= 1.0f ? 255 : (uint8_t)std::floor(c * 255.0f + 0.5f);
                }
            } else px = r.ReadFramebufferRgba8();
            FILE *f = std::fopen(ppm.c_str(), "wb");
            if (!f) throw std::runtime_error("cannot open " + ppm);
            std::fprintf(f, "P6\n%u %u\n255\n", w, h);
            for (size_t i = 0; i < px.size(); i += 4) std::fwrite(&px[i], 1, 3, f);
            std::fclose(f);
        }
        if (!pfm.empty()) { // linear float radiance, bottom-up rows, little endian
            const auto px = denoise >= 0 ? denoised : r.ReadFramebuffer();
            FILE *f = std::fopen(pfm.c_str(), "wb");
            if (!f) throw std::runtime_error("cannot open " + pfm);
            std::fprintf(f, "PF\n%u %u\n-1.0\n", w, h);
            for (uint32_t y = h; y-- > 0;)
                for (uint32_t x = 0; x < w; ++x) std::fwrite(&px[((size_t)y * w + x) * 4], 4, 3, f);
            std::fclose(f);
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "ptrt_cli: %s\n", e.what());
        return 1;
    }
    return 0;
}
