// scene.h — pt_scene, and one owner each for the things a committed scene keeps on both sides of the bus: its tree, its vertices and its
// textures. Which copy is current is private to the owner; nobody else keeps a flag about it. Private to scene.cpp, frame.cpp,
// query.cpp and denoise_host.cpp; the context a scene belongs to and the helpers every public call uses are context.h's.
#pragma once
#include "context.h"
#include "bvh_build.h"
#include "blob_rules.h"
#include "environment.h"
#include <vector>

namespace ptrt {

struct CommitClock;

uint64_t next_scene_serial(); // never the same value twice in a process (scene.cpp)

// The committed tree: the device arrays the kernels traverse, its figures (recorded when the tree is adopted, never re-derived), and the
// host image of the docs/SPEC.md §4.1 blob. The image is fresh after a host build, lacks current boxes and triangle rows after a refit,
// and is absent after a build that packed the blob on the device; host_image() fetches exactly then.
class CommittedTree {
public:
    DevBuf<float4> d_nodes, d_tris;      // nodes in the layout's format; one 64-byte record per blob triangle
    uint32_t layout = 0, fan = 0;        // PT_BVH_WIDTH_* the scene was committed with, children per node
    uint32_t n_nodes = 0, n_tris = 0;    // n_tris: blob triangle records
    uint32_t max_depth = 0, stack_need = 0;
    float sah_cost = 0.f;
    double build_ms = 0.0;
    uint64_t node_bytes = 0;
    uint32_t stack_overflow() const { return stack_need > kStackLds ? stack_need - kStackLds : 0u; } // traversal-stack entries per ray beyond those in LDS

    // A host-built blob (quantised here where the layout wants it): the image is fresh, the upload pending. The device arrays of the
    // tree before it stay for upload() to reuse.
    void adopt(BvhBlob &&blob, uint32_t layout_id);
    // A BVH4Q blob packed on the device (lbvh.hip build_lbvh_blob4q_device) over n_records triangles: no image, nothing to upload
    void adopt(DeviceBlob4Q &&blob, uint32_t n_records);
    pt_status upload(pt_context *c, CommitClock &clock);
    // The refit rewrote every box and triangle row of the device copy. Refs and ids stay: an update never changes the topology.
    void device_rewritten(float new_sah_cost) { sah_cost = new_sah_cost; if (image == Image::fresh) image = Image::topology_only; }
    pt_status host_image(pt_context *c, const void *&nodes, const BvhTri *&tris) const;
    // Narrow reads of the topology, 4 bytes per child slot / per record, from the image if it has them, else by a strided copy:
    // the refs of every node (n_nodes x fan) and the original triangle id of every blob record
    pt_status refs(pt_context *c, std::vector<int32_t> &out) const;
    pt_status ids(pt_context *c, std::vector<uint32_t> &out) const;
    // The union of the root node's child boxes as the device copy holds them (decoded as the kernels decode them): every ray that
    // reaches a triangle has passed the slab test of one of them. Kept current by whoever rewrites the device copy: bound_stale()
    // before the first write, fetch_root() enqueued behind the last one, root_fetched() once the stream has been waited for. A tree
    // without nodes has the empty box. False while stale: the caller then assumes nothing about where the triangles are.
    void bound_stale() { bound_valid = false; }
    hipError_t fetch_root(hipStream_t q);
    void root_fetched();
    bool root_bound(Box &out) const { out = bound; return bound_valid; }

private:
    Box bound = Box::empty();
    bool bound_valid = false;
    uint8_t root_bytes[256] = {};        // node 0 as fetch_root() copied it (the largest node, BVH4 / BVH8Q, has 128 bytes)
    enum class Image { fresh, topology_only, absent };
    mutable Image image = Image::fresh;  // (mutable with the vectors below: pt_scene_bvh_read fills them through a const scene)
    mutable std::vector<BvhSlot> slots;  // f32 layouts: n_nodes * fan
    mutable std::vector<uint8_t> packed; // layouts PT_BVH_WIDTH_4Q / _8Q / _8O: the 64- / 128-byte nodes
    mutable std::vector<BvhTri> tris;
    bool upload_pending = false;
    const void *node_data() const { return layout_quantised(layout) ? (const void *)packed.data() : (const void *)slots.data(); }
};

// A scene's triangle vertices (9 floats each): the host vector and the two device buffers updates alternate between. An update
// writes next(), and only when all of it has succeeded does next_is_current() make that the scene's vertices.
class SceneVertices {
public:
    void set(const float *verts9, uint64_t count) { host_.assign(verts9, verts9 + count * 9); host_stale = false; dev_current = false; }
    pt_status host(pt_context *c, const float *&verts9); // fetched first if an update has run since
    // the current vertices on the device: the host vector is uploaded once if no update has run yet (const: pt_denoise_temporal asks
    // through the const scene it receives, and the scene's vertices stay what they are)
    pt_status device(pt_context *c, const float *&verts9) const;
    hipError_t reserve_device()                          // both buffers, for as many vertices as the host vector holds
    {
        const hipError_t e = dev[0].ensure(host_.size());
        return e != hipSuccess ? e : dev[1].ensure(host_.size());
    }
    float *next() const { return dev[cur ^ 1u].p; }
    void next_is_current() { cur ^= 1u; host_stale = true; dev_current = true; }

private:
    std::vector<float> host_;
    mutable DevBuf<float> dev[2];
    uint32_t cur = 0;        // dev[cur] holds the scene's vertices while host_stale
    bool host_stale = false;
    mutable bool dev_current = false; // dev[cur] holds the scene's vertices (an update's, or device()'s upload of the host vector)
};

// A scene's albedo textures (docs/SPEC.md §13): the per-triangle UVs, the textures and the per-material binding as the three setters left
// them (host side, scene content like the triangles: they take effect with pt_scene_commit), and the one device copy of each that a commit
// of a textured scene makes — the UV rows in blob order with every triangle's material resolved to its texture, the descriptors and the
// texels. Whether the committed scene is textured is this owner's to say; nobody else keeps a flag about it.
class SceneTextures {
public:
    struct Texture { uint32_t width = 0, height = 0, flags = 0; std::vector<float> rgb; }; // width 0: not set
    std::vector<float> uvs;                  // 6 floats per triangle; empty with !have_uvs
    bool have_uvs = false;
    Texture tex[PT_MAX_TEXTURES];
    std::vector<uint32_t> of_material;       // a texture index or PT_NO_TEXTURE per material; empty with !have_binding
    bool have_binding = false;

    // pt_scene_commit's check: the counts against the scene's, every bound index against the textures that are set
    pt_status check(pt_context *c, size_t n_tris, size_t n_mats) const;
    // pt_scene_commit: decides textured() for the scene being committed and, with a context, builds and uploads the device copy from the
    // committed tree's original ids (blob order) and the triangles' materials
    pt_status commit(pt_context *c, const std::vector<uint32_t> &tri_mat, const CommittedTree &tree);
    bool textured() const { return textured_; }
    TexArgs args() const { return TexArgs{ d_uv.p, d_desc.p, d_texels.p, n_desc, 0u }; }
    uint64_t device_bytes(uint32_t index) const { return dev_bytes[index]; }
    uint32_t bound_materials(uint32_t index) const;

private:
    bool textured_ = false;
    uint32_t n_desc = 0;
    uint64_t dev_bytes[PT_MAX_TEXTURES] = {};
    DevBuf<float4> d_uv, d_texels;
    DevBuf<uint4> d_desc;
};

struct ExtendChoice {           // what a scene remembers of the extend-kernel probe (frame.cpp ExtendFrame)
    uint32_t kernel = 0;        // the ExtendKernel an earlier frame picked (0 = none yet)
    double rate_simple = 0.0, rate_packed = 0.0; // rays per ms of whole frames run on one kernel (frames too short to probe inside)
    uint32_t misses = 0;        // warm frames too small to time: after three the scene settles on the one-ray-per-lane kernel for good
};

// Everything derived from the committed tree and filled on first use, not scene content: pt_scene_commit forgets it all at once. The
// device buffers keep their allocations across commits (ensure()); only what they hold stops counting.
struct CommitCaches {
    // pt_scene_update_triangles (refit.hip, docs/SPEC.md §4.3): made by the first update after a commit
    struct Refit {
        bool ready = false;                  // level lists built for the committed tree
        std::vector<uint32_t> level_off;     // level l (deepest first) = list[level_off[l] .. level_off[l + 1])
        DevBuf<uint32_t> list, flag;
        DevBuf<float> tbox, nbox, carea;     // per blob triangle / per node / per child slot
        DevBuf<double> sah;                  // per-block partial sums, then the total
        Event ev[4];
    } refit;
    // pt_denoise: original triangle id -> blob index (where a guide finds its hit's shading row), made by the first denoise after a
    // commit; updates keep it (they keep every record's id and place)
    DevBuf<uint32_t> d_blob_of;
    bool blob_of_ready = false;
    ExtendChoice ext;                        // what earlier frames measured
    void invalidate() { refit.ready = false; blob_of_ready = false; ext = ExtendChoice{}; }
};

} // namespace ptrt

struct pt_scene {
    pt_context *ctx = nullptr;
    // Which committed geometry this is, for whoever keeps something derived from it across calls (context.h TemporalHistory's
    // snapshot): `serial` is unique per scene object and per pt_scene_commit, `updates` counts the geometry updates since.
    uint64_t serial = ptrt::next_scene_serial(), updates = 0;
    ptrt::SceneVertices verts; std::vector<uint32_t> tri_mat;
    std::vector<float> spheres; std::vector<uint32_t> sph_mat;
    std::vector<pt_material> mats;
    pt_camera cam{};
    float sky[3] = { 0.f, 0.f, 0.f };
    ptrt::Environment env;               // while present it replaces `sky` on the misses of a path-traced frame (docs/SPEC.md §11); not
                                         // scene content in the commit's sense: set, replaced and removed at any time, kept by commits and updates
    pt_lens lens{};                      // pt_scene_set_lens (docs/SPEC.md §3.1); radius 0 = none. Like `sky` host values only, read by every pt_render:
                                         // set and removed at any time, kept by commits, updates and pt_scene_set_camera
    ptrt::SceneTextures textures;        // pt_scene_set_triangle_uvs / _texture / _material_textures (docs/SPEC.md §13)
    bool have_cam = false, committed = false;
    ptrt::CommittedTree tree;
    mutable ptrt::CommitCaches cache;    // (mutable: pt_render and pt_denoise fill it through the const scene they receive)
    ptrt::DevBuf<float4> d_spheres, d_mats;
    bool has_specular = false;
    ptrt::DevBuf<uint2> d_sph_mat;
    ptrt::DeviceScene ds{};
    // The light table of next-event estimation (docs/SPEC.md §7, build_lights): made at every commit and every triangle update from the
    // candidates — the triangles whose material emits, in triangle order — of which those with area * (e.r + e.g + e.b) > 0 are lights.
    std::vector<uint32_t> light_cand;    // original ids of the candidates
    std::vector<uint32_t> cand_blob;     // the blob index of each candidate (where its pa goes in d_pa)
    std::vector<float> pa_span;          // host image of d_pa[cand_lo .. cand_hi], the only entries that can be non-zero
    uint32_t cand_lo = 0, n_lights = 0;
    ptrt::DevBuf<float4> d_lights;
    ptrt::DevBuf<float> d_cdf, d_pa;
    // The joint table of docs/SPEC.md §7.1 (build_sphere_lights), beside the one above and only while the scene has a sphere light: the triangle
    // lights with their joint pa, then the spheres whose material emits and whose 2 pi r^2 (e.r + e.g + e.b) > 0, in sphere order. Made
    // wherever the table above is made and at every pt_scene_update_spheres, from what build_lights kept of the triangle side.
    std::vector<double> light_w;         // per triangle light: its weight area * (e.r + e.g + e.b)
    std::vector<float> light_area;       // ... its area
    std::vector<float> light_rec;        // ... its 16-float record (with the triangle table's own pa)
    std::vector<uint32_t> light_blob;    // ... its blob index
    uint32_t n_sph_lights = 0;           // 0: no joint table; flagged calls are the unflagged ones
    bool jpa_zeroed = false;             // d_jpa has its size and its zeroes for this commit
    ptrt::DevBuf<float4> d_jlights;      // n_lights + n_sph_lights records
    ptrt::DevBuf<float> d_jcdf, d_jpa, d_sph_pmf; // d_jpa: per blob triangle like d_pa; d_sph_pmf: per sphere, 0 for a sphere that is no light
};

// Not part of include/ptrt.h: the binary tree of build_lbvh_device, read out for the test suite (tests/test_gpu_lbvh.py compares it with a
// plain reference). Runs on the context's stream; order[n], left/right/first/last[n - 1] and box6[6 * (n - 1)] are the fields of BinaryBvh.
// PT_ERR_INVALID_ARGUMENT for n < 2, a NULL pointer and, as pt_scene_set_triangles refuses them before a commit, n >= 2^28 or a non-finite
// coordinate.
extern "C" pt_status pt_internal_lbvh_binary(pt_context *ctx, const float *verts9, uint64_t n, uint32_t *order, int32_t *left, int32_t *right,
                                             uint32_t *first, uint32_t *last, float *box6);
