// scene.cpp — the scene half of the C ABI (include/ptrt.h): pt_scene's contents, pt_scene_commit in phases, the blob read-back, geometry
// updates; and the two owners of scene.h.
#include "scene.h"
#include "refit.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

using namespace ptrt;

// ------------------------------------------------------------------------------------------------ the owners (scene.h)

struct ptrt::CommitClock { // PTRT_TIMING (developer aid): where a commit's time goes, on stderr
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void lap(const char *what)
    {
        static const bool timing = getenv("PTRT_TIMING") != nullptr;
        if (timing) fprintf(stderr, "ptrt commit: %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count());
        t = std::chrono::steady_clock::now();
    }
};

void CommittedTree::adopt(BvhBlob &&blob, uint32_t layout_id)
{
    layout = layout_id; fan = blob.width; n_nodes = blob.n_nodes; n_tris = (uint32_t)blob.tris.size();
    max_depth = blob.max_depth; stack_need = blob.stack_need; sah_cost = blob.sah_cost; build_ms = blob.build_ms;
    packed.clear();
    if (layout_quantised(layout)) {
        if (fan == 4) quantize_bvh4(blob, packed);
        else quantize_bvh8(blob, packed);
    }
    slots = std::move(blob.slots); tris = std::move(blob.tris);
    node_bytes = layout_quantised(layout) ? packed.size() : slots.size() * sizeof(BvhSlot);
    image = Image::fresh; upload_pending = true; bound_valid = false;
}

void CommittedTree::adopt(DeviceBlob4Q &&blob, uint32_t n_records)
{
    d_nodes = std::move(blob.nodes); d_tris = std::move(blob.tris); // (the arrays of the tree before it are freed here)
    layout = PT_BVH_WIDTH_4Q; fan = layout_fan(layout); n_nodes = blob.n_nodes; n_tris = n_records;
    max_depth = blob.max_depth; stack_need = blob.stack_need; sah_cost = blob.sah_cost; build_ms = blob.device_ms;
    node_bytes = (uint64_t)n_nodes * layout_node_bytes(layout);
    slots.clear(); packed.clear(); tris.clear();
    image = Image::absent; upload_pending = false; bound_valid = false;
}

pt_status CommittedTree::upload(pt_context *c, CommitClock &clock)
{
    // the traversal kernels fetch a node or a triangle record by a 32-bit byte offset from its array's base (kernels.hip record())
    if (node_bytes > (1ull << 32) || (uint64_t)n_tris * 64u > (1ull << 32))
        return fail(c, PT_ERR_UNSUPPORTED, "BVH of %llu node bytes and %llu triangle records: each array must stay within 4 GiB",
                    (unsigned long long)node_bytes, (unsigned long long)n_tris);
    HIP_TRY(c, hipSetDevice(context_device(c)));
    static_assert(sizeof(BvhSlot) == 32 && sizeof(BvhTri) == 48 && sizeof(pt_material) == 48, "blob layout");
    if (!upload_pending) return PT_OK;
    HIP_TRY(c, d_nodes.ensure((size_t)(node_bytes / 16)));
    HIP_TRY(c, d_tris.ensure(tris.size() * 4));
    // Device triangle record = one 64-byte line: the blob's three rows (docs/SPEC.md §4.1) + a shading row. A 48-byte
    // record straddles two cache lines 3 times out of 4 when k_extend fetches it; a padded one never does, and the
    // row that pads it is the one k_shade wants next: ng and the material id (blob_rules.h shading_row; rows 0-2 are the blob's triangle).
    std::vector<float> rec(tris.size() * 16);
    for (size_t i = 0; i < tris.size(); ++i) {
        const BvhTri &t = tris[i];
        std::memcpy(&rec[i * 16], &t, sizeof(BvhTri));
        shading_row(t.e1, t.e2, t.mat, &rec[i * 16 + 12]);
    }
    clock.lap("triangle records");
    if (!rec.empty()) HIP_TRY(c, hipMemcpy(d_tris.p, rec.data(), rec.size() * sizeof(float), hipMemcpyHostToDevice));
    clock.lap("upload triangles");
    if (node_bytes) HIP_TRY(c, hipMemcpy(d_nodes.p, node_data(), node_bytes, hipMemcpyHostToDevice));
    upload_pending = false;
    return PT_OK;
}

pt_status CommittedTree::host_image(pt_context *c, const void *&nodes, const BvhTri *&tris48) const
{
    if (image != Image::fresh) { // fetch the blob now: nodes as they are, triangles = rows 0-2 of the 64-byte records
        HIP_TRY(c, hipSetDevice(context_device(c)));
        if (layout_quantised(layout)) packed.resize(node_bytes);
        else slots.resize((size_t)n_nodes * fan);
        std::vector<float> rec((size_t)n_tris * 16);
        if (node_bytes) HIP_TRY(c, hipMemcpy(const_cast<void *>(node_data()), d_nodes.p, node_bytes, hipMemcpyDeviceToHost));
        if (!rec.empty()) HIP_TRY(c, hipMemcpy(rec.data(), d_tris.p, rec.size() * sizeof(float), hipMemcpyDeviceToHost));
        tris.resize(n_tris);
        for (size_t i = 0; i < tris.size(); ++i) std::memcpy(&tris[i], &rec[i * 16], sizeof(BvhTri));
        image = Image::fresh;
    }
    nodes = node_data(); tris48 = tris.data();
    return PT_OK;
}

pt_status CommittedTree::refs(pt_context *c, std::vector<int32_t> &out) const
{
    const uint32_t stride = layout_node_bytes(layout);
    out.resize((size_t)n_nodes * fan);
    if (image == Image::absent) { // packed on the device, so quantised: the refs are one run in every node
        if (n_nodes) HIP_TRY(c, hipMemcpy2D(out.data(), 4 * fan, (const uint8_t *)d_nodes.p + layout_ref_at(layout, 0), stride, 4 * fan, n_nodes, hipMemcpyDeviceToHost));
        return PT_OK;
    }
    const uint8_t *nd = (const uint8_t *)node_data();
    for (size_t i = 0; i < n_nodes; ++i)
        for (uint32_t k = 0; k < fan; ++k) std::memcpy(&out[i * fan + k], nd + i * stride + layout_ref_at(layout, k), 4);
    return PT_OK;
}

pt_status CommittedTree::ids(pt_context *c, std::vector<uint32_t> &out) const
{
    out.resize(n_tris);
    if (image == Image::absent) { if (n_tris) HIP_TRY(c, hipMemcpy2D(out.data(), 4, (const uint8_t *)d_tris.p + 12, 64, 4, n_tris, hipMemcpyDeviceToHost)); } // row 0 .w
    else for (uint32_t j = 0; j < n_tris; ++j) out[j] = tris[j].id;
    return PT_OK;
}

hipError_t CommittedTree::fetch_root(hipStream_t q)
{
    if (!n_nodes) return hipSuccess;
    if (layout_node_bytes(layout) > sizeof root_bytes) return hipErrorInvalidValue;
    return hipMemcpyAsync(root_bytes, d_nodes.p, layout_node_bytes(layout), hipMemcpyDeviceToHost, q);
}

void CommittedTree::root_fetched()
{
    bound = Box::empty();
    if (n_nodes) {
        uint32_t w[sizeof root_bytes / 4];
        std::memcpy(w, root_bytes, sizeof root_bytes);
        for (uint32_t c = 0; c < fan; ++c) {
            int32_t ref; std::memcpy(&ref, root_bytes + layout_ref_at(layout, c), 4);
            if (ref == kEmptyRef) continue;
            Box b;
            if (layout_quantised(layout)) { // docs/SPEC.md §4.1: fma((float)q, 2^e, origin), the q of child c in byte c of its coordinate group
                const uint32_t kw = fan / 4u, q0 = 4u + fan;
                for (uint32_t a = 0; a < 3; ++a) {
                    const float org = bits_as_float(w[a]), sc = quant_scale_of((w[3] >> (8u * a)) & 0xffu);
                    const uint32_t ql = (w[q0 + kw * a + c / 4u] >> (8u * (c % 4u))) & 0xffu, qh = (w[q0 + kw * (3u + a) + c / 4u] >> (8u * (c % 4u))) & 0xffu;
                    b.lo[a] = __builtin_fmaf((float)ql, sc, org); b.hi[a] = __builtin_fmaf((float)qh, sc, org);
                }
            } else {
                BvhSlot sl; std::memcpy(&sl, root_bytes + 32u * c, sizeof sl);
                for (int a = 0; a < 3; ++a) { b.lo[a] = sl.lo[a]; b.hi[a] = sl.hi[a]; }
            }
            bound.grow(b);
        }
    }
    bound_valid = true;
}

pt_status SceneVertices::host(pt_context *c, const float *&verts9)
{
    if (host_stale) {
        HIP_TRY(c, hipSetDevice(context_device(c)));
        HIP_TRY(c, hipMemcpy(host_.data(), dev[cur].p, host_.size() * sizeof(float), hipMemcpyDeviceToHost));
        host_stale = false;
    }
    verts9 = host_.data();
    return PT_OK;
}

pt_status SceneVertices::device(pt_context *c, const float *&verts9) const
{
    if (!dev_current) {
        HIP_TRY(c, hipSetDevice(context_device(c)));
        HIP_TRY(c, dev[cur].ensure(host_.size()));
        if (!host_.empty()) HIP_TRY(c, hipMemcpy(dev[cur].p, host_.data(), host_.size() * sizeof(float), hipMemcpyHostToDevice));
        dev_current = true;
    }
    verts9 = dev[cur].p;
    return PT_OK;
}

pt_status SceneTextures::check(pt_context *c, size_t n_tris, size_t n_mats) const
{
    if (have_uvs && uvs.size() != n_tris * 6)
        return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_scene_set_triangle_uvs gave %llu triangles, the scene has %llu", (unsigned long long)(uvs.size() / 6), (unsigned long long)n_tris);
    if (have_binding) {
        if (of_material.size() != n_mats)
            return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_scene_set_material_textures gave %llu materials, the scene has %llu", (unsigned long long)of_material.size(), (unsigned long long)n_mats);
        for (size_t m = 0; m < n_mats; ++m) {
            const uint32_t t = of_material[m];
            if (t != PT_NO_TEXTURE && (t >= PT_MAX_TEXTURES || tex[t].width == 0))
                return fail(c, PT_ERR_INVALID_ARGUMENT, "material %llu is bound to texture %u, which is not set", (unsigned long long)m, t);
        }
    }
    return PT_OK;
}

uint32_t SceneTextures::bound_materials(uint32_t index) const
{
    uint32_t n = 0;
    if (have_binding) for (const uint32_t t : of_material) n += t == index ? 1u : 0u;
    return n;
}

pt_status SceneTextures::commit(pt_context *c, const std::vector<uint32_t> &tri_mat, const CommittedTree &tree)
{
    textured_ = false; n_desc = 0;
    for (uint64_t &b : dev_bytes) b = 0;
    // the textures some material is bound to, in index order: descriptor `desc_of[t]`
    uint32_t desc_of[PT_MAX_TEXTURES];
    std::vector<uint32_t> used;
    for (uint32_t t = 0; t < PT_MAX_TEXTURES; ++t) {
        desc_of[t] = PT_NO_TEXTURE;
        if (tex[t].width && bound_materials(t)) { desc_of[t] = (uint32_t)used.size(); used.push_back(t); }
    }
    if (!have_uvs || tri_mat.empty() || used.empty()) return PT_OK; // not textured: no kernel of §13 runs, nothing is uploaded
    textured_ = true;
    if (!c) return PT_OK;                                           // detached scene: host side only
    std::vector<uint32_t> ids;
    const pt_status st = tree.ids(c, ids);
    if (st != PT_OK) return st;
    // UV rows in blob order, the triangle's material resolved to its descriptor
    std::vector<float> rows(ids.size() * 8);
    for (size_t j = 0; j < ids.size(); ++j) {
        const uint32_t id = ids[j] < tri_mat.size() ? ids[j] : 0u, t = of_material[tri_mat[id]];
        const uint32_t di = t == PT_NO_TEXTURE ? PT_NO_TEXTURE : desc_of[t];
        std::memcpy(&rows[j * 8], &uvs[(size_t)id * 6], 6 * sizeof(float));
        std::memcpy(&rows[j * 8 + 6], &di, 4);
        rows[j * 8 + 7] = 0.f;
    }
    std::vector<uint4> desc(used.size());
    uint64_t total = 0;
    for (size_t k = 0; k < used.size(); ++k) {
        const Texture &T = tex[used[k]];
        desc[k] = uint4{ (uint32_t)total, T.width, T.height, T.flags };
        total += (uint64_t)T.width * T.height; // <= 64 * 2^24 texels: the first texel fits 32 bits
        dev_bytes[used[k]] = (uint64_t)T.width * T.height * sizeof(float4);
    }
    HIP_TRY(c, hipSetDevice(context_device(c)));
    HIP_TRY(c, d_uv.ensure(rows.size() / 4)); HIP_TRY(c, d_desc.ensure(desc.size())); HIP_TRY(c, d_texels.ensure((size_t)total));
    HIP_TRY(c, hipMemcpy(d_uv.p, rows.data(), rows.size() * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(d_desc.p, desc.data(), desc.size() * sizeof(uint4), hipMemcpyHostToDevice));
    std::vector<float> t4;
    for (size_t k = 0; k < used.size(); ++k) { // one texture at a time: the staging copy stays one texture large
        const Texture &T = tex[used[k]];
        const size_t n = (size_t)T.width * T.height;
        t4.assign(n * 4, 0.f);
        for (size_t i = 0; i < n; ++i) { t4[i * 4] = T.rgb[i * 3]; t4[i * 4 + 1] = T.rgb[i * 3 + 1]; t4[i * 4 + 2] = T.rgb[i * 3 + 2]; }
        HIP_TRY(c, hipMemcpy(d_texels.p + desc[k].x, t4.data(), n * sizeof(float4), hipMemcpyHostToDevice));
    }
    n_desc = (uint32_t)used.size();
    return PT_OK;
}

uint64_t ptrt::next_scene_serial()
{
    static std::atomic<uint64_t> last{ 0 };
    return ++last;
}

// ------------------------------------------------------------------------------------------------ scene contents

namespace {

bool finite3(const float *p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }
bool sphere_ok(const float *cxyzr) { return finite3(cxyzr) && cxyzr[3] > 0.f && std::isfinite(cxyzr[3]); } // finite centre, finite radius > 0

// The device's {material id, bits of 1.0f / r} per sphere (IEEE single division: the value docs/SPEC.md §5 has the shading step compute)
std::vector<uint2> sphere_mats(const uint32_t *mat, const float *cxyzr, size_t n)
{
    std::vector<uint2> mi(n);
    for (size_t i = 0; i < n; ++i) { const float inv_r = 1.0f / cxyzr[i * 4 + 3]; mi[i].x = mat[i]; std::memcpy(&mi[i].y, &inv_r, 4); }
    return mi;
}

// docs/SPEC.md §7.1: the joint table — the triangle lights build_lights kept (s->light_*), then the scene's sphere lights in sphere order —
// with one running sum in double, uploaded beside the triangle table. Without a sphere light there is none (n_sph_lights = 0).
static pt_status build_sphere_lights(pt_context *c, pt_scene *s)
{
    const size_t ns = s->sph_mat.size(), nt = s->light_w.size();
    std::vector<double> w(s->light_w);
    std::vector<float> rec(s->light_rec), pmf_of(std::max<size_t>(ns, 1), 0.0f);
    std::vector<uint32_t> sph; // which sphere each sphere light is
    for (size_t j = 0; j < ns; ++j) {
        const float *e = s->mats[s->sph_mat[j]].emission, *cr = s->spheres.data() + j * 4;
        if (e[0] == 0.f && e[1] == 0.f && e[2] == 0.f) continue;
        const double wj = (6.283185307179586 * ((double)cr[3] * (double)cr[3])) * (((double)e[0] + (double)e[1]) + (double)e[2]);
        if (!(wj > 0.0)) continue;
        w.push_back(wj); sph.push_back((uint32_t)j);
        float lamp; // the bits of 1 + j: which sphere a pending shadow ray goes to
        const uint32_t lamp_bits = (uint32_t)j + 1u; std::memcpy(&lamp, &lamp_bits, 4);
        const float r[16] = { cr[0], cr[1], cr[2], 0.f, cr[3], lamp, 0.f, e[0], 0.f, 0.f, 0.f, e[1], 0.f, 0.f, 0.f, e[2] };
        rec.insert(rec.end(), r, r + 16);
    }
    s->n_sph_lights = (uint32_t)sph.size();
    if (sph.empty() || !c) return PT_OK;
    const size_t nl = w.size();
    double total = 0.0, run = 0.0;
    for (const double wi : w) total += wi;
    std::vector<float> cdf(nl), jpa(s->pa_span.size(), 0.0f);
    for (size_t i = 0; i < nl; ++i) {
        run += w[i]; // the same sums in the same order as above
        cdf[i] = i + 1 == nl ? 1.0f : (float)(run / total);
        const float pmf = (float)(w[i] / total);
        if (i < nt) { rec[i * 16 + 3] = pmf / s->light_area[i]; jpa[s->light_blob[i] - s->cand_lo] = rec[i * 16 + 3]; }
        else { rec[i * 16 + 3] = pmf; pmf_of[sph[i - nt]] = pmf; }
    }
    if (!s->jpa_zeroed) {
        const size_t nbt = std::max<size_t>(s->tree.n_tris, 1);
        HIP_TRY(c, s->d_jpa.ensure(nbt)); HIP_TRY(c, hipMemset(s->d_jpa.p, 0, nbt * sizeof(float)));
        s->jpa_zeroed = true;
    }
    HIP_TRY(c, s->d_jlights.ensure(nl * 4)); HIP_TRY(c, s->d_jcdf.ensure(nl)); HIP_TRY(c, s->d_sph_pmf.ensure(pmf_of.size()));
    HIP_TRY(c, hipMemcpy(s->d_jlights.p, rec.data(), rec.size() * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(s->d_jcdf.p, cdf.data(), nl * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(s->d_sph_pmf.p, pmf_of.data(), pmf_of.size() * sizeof(float), hipMemcpyHostToDevice));
    if (!jpa.empty()) HIP_TRY(c, hipMemcpy(s->d_jpa.p + s->cand_lo, jpa.data(), jpa.size() * sizeof(float), hipMemcpyHostToDevice));
    return PT_OK;
}

// docs/SPEC.md §7: the light set, its f32 CDF and the per-light records from the current vertices of the candidates, uploaded to the
// scene's device arrays. `verts` holds the triangles from `first` on (9 floats each, in triangle order). Area, normal and pa in the op
// order of §0 / §7; the weights in double.
pt_status build_lights(pt_context *c, pt_scene *s, const float *verts, uint32_t first)
{
    std::vector<float> rec, cdf; // 16 floats per light: v0|pa, e1|Le.r, e2|Le.g, n_l|Le.b
    std::vector<double> w;       // area * (e.r + e.g + e.b) per light
    std::vector<uint32_t> cand;  // which candidate each light is
    std::vector<float> areas;
    double total = 0.0;
    for (size_t k = 0; k < s->light_cand.size(); ++k) {
        const float *v = verts + (size_t)(s->light_cand[k] - first) * 9;
        const float e1[3] = { v[3] - v[0], v[4] - v[1], v[5] - v[2] }, e2[3] = { v[6] - v[0], v[7] - v[1], v[8] - v[2] };
        float nl[3]; // n_l: the bits of the shading row
        const float area = 0.5f * std::sqrt(shading_normal(e1, e2, nl));
        const float *e = s->mats[s->tri_mat[s->light_cand[k]]].emission;
        const double wk = (double)area * ((double)e[0] + (double)e[1] + (double)e[2]);
        if (!(area > 0.f) || !(wk > 0.0)) continue;
        total += wk; w.push_back(wk); cand.push_back((uint32_t)k); areas.push_back(area);
        const float r[16] = { v[0], v[1], v[2], area, e1[0], e1[1], e1[2], e[0], e2[0], e2[1], e2[2], e[1], nl[0], nl[1], nl[2], e[2] };
        rec.insert(rec.end(), r, r + 16);
    }
    const size_t nl = w.size();
    cdf.resize(nl);
    std::fill(s->pa_span.begin(), s->pa_span.end(), 0.0f);
    double run = 0.0;
    for (size_t i = 0; i < nl; ++i) {
        run += w[i]; // the same sums in the same order as above
        cdf[i] = i + 1 == nl ? 1.0f : (float)(run / total);
        const float pa = (float)(w[i] / total) / rec[i * 16 + 3]; // pmf (as stored, f32) / area
        rec[i * 16 + 3] = pa;
        s->pa_span[s->cand_blob[cand[i]] - s->cand_lo] = pa;
    }
    s->n_lights = (uint32_t)nl;
    s->light_w = w; s->light_area = areas; s->light_rec = rec; s->light_blob.resize(nl); // §7.1: what the joint table takes from this one
    for (size_t i = 0; i < nl; ++i) s->light_blob[i] = s->cand_blob[cand[i]];
    if (!c) return build_sphere_lights(c, s); // (no device copy; the counts stay consistent)
    HIP_TRY(c, s->d_lights.ensure(std::max<size_t>(nl, 1) * 4)); HIP_TRY(c, s->d_cdf.ensure(std::max<size_t>(nl, 1)));
    if (nl) {
        HIP_TRY(c, hipMemcpy(s->d_lights.p, rec.data(), rec.size() * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(s->d_cdf.p, cdf.data(), nl * sizeof(float), hipMemcpyHostToDevice));
    }
    if (!s->pa_span.empty()) HIP_TRY(c, hipMemcpy(s->d_pa.p + s->cand_lo, s->pa_span.data(), s->pa_span.size() * sizeof(float), hipMemcpyHostToDevice));
    return build_sphere_lights(c, s);
}

} // namespace

extern "C" {

pt_status pt_scene_create(pt_context *ctx, pt_scene **out)
{
    // ctx == NULL makes a detached (host-only) scene: commit builds the BVH blob for pt_scene_bvh_read/info,
    // nothing is uploaded and pt_render rejects it. Used to check the builder where no device exists.
    if (!out) return fail(ctx, PT_ERR_INVALID_ARGUMENT, "pt_scene_create: NULL argument");
    pt_scene *s = new (std::nothrow) pt_scene();
    if (!s) return fail(ctx, PT_ERR_OUT_OF_MEMORY, "host allocation failed");
    s->ctx = ctx;
    *out = s;
    return PT_OK;
}

void pt_scene_destroy(pt_scene *s)
{
    if (!s) return;
    if (s->ctx) { (void)hipSetDevice(s->ctx->device); (void)hipStreamSynchronize(s->ctx->stream); }
    delete s;
}

pt_status pt_scene_set_triangles(pt_scene *s, const float *verts9, const uint32_t *material_ids, uint64_t count)
{
    if (!s) return fail(nullptr, PT_ERR_INVALID_ARGUMENT, "scene is NULL");
    if (count && !verts9) return fail(s->ctx, PT_ERR_INVALID_ARGUMENT, "verts9 is NULL");
    if (count >= (1ull << 28)) return fail(s->ctx, PT_ERR_UNSUPPORTED, "more than 2^28 triangles");
    for (uint64_t i = 0; i < count * 9; ++i)
        if (!std::isfinite(verts9[i])) return fail(s->ctx, PT_ERR_INVALID_ARGUMENT, "non-finite vertex coordinate at float %llu", (unsigned long long)i);
    s->verts.set(verts9, count);
    if (material_ids) s->tri_mat.assign(material_ids, material_ids + count); else s->tri_mat.assign(count, 0u);
    s->committed = false;
    return PT_OK;
}

pt_status pt_scene_set_spheres(pt_scene *s, const float *cxyzr, const uint32_t *material_ids, uint64_t count)
{
    if (!s) return fail(nullptr, PT_ERR_INVALID_ARGUMENT, "scene is NULL");
    if (count && !cxyzr) return fail(s->ctx, PT_ERR_INVALID_ARGUMENT, "cxyzr is NULL");
    if (count > kMaxSpheres) return fail(s->ctx, PT_ERR_UNSUPPORTED, "more than %u spheres (they are a flat list)", kMaxSpheres);
    for (uint64_t i = 0; i < count; ++i)
        if (!sphere_ok(cxyzr + i * 4)) return fail(s->ctx, PT_ERR_INVALID_ARGUMENT, "sphere %llu: non-finite centre or radius <= 0", (unsigned long long)i);
    s->spheres.assign(cxyzr, cxyzr + count * 4);
    if (material_ids) s->sph_mat.assign(material_ids, material_ids + count); else s->sph_mat.assign(count, 0u);
    s->committed = false;
    return PT_OK;
}

pt_status pt_scene_set_materials(pt_scene *s, const pt_material *mats, uint64_t count)
{
    if (!s) return fail(nullptr, PT_ERR_INVALID_ARGUMENT, "scene is NULL");
    if (count && !mats) return fail(s->ctx, PT_ERR_INVALID_ARGUMENT, "mats is NULL");
    for (uint64_t i = 0; i < count; ++i) {
        if (mats[i].kind > PT_DIELECTRIC) return fail(s->ctx, PT_ERR_INVALID_ARGUMENT, "material %llu: unknown kind %u", (unsigned long long)i, mats[i].kind);
        if (!finite3(mats[i].albedo) || !finite3(mats[i].emission) || !std::isfinite(mats[i].roughness) || !std::isfinite(mats[i].ior))
            return fail(s->ctx, PT_ERR_INVALID_ARGUMENT, "material %llu: non-finite field", (unsigned long long)i);
        if (mats[i].roughness < 0.f || mats[i].roughness > 1.f) return fail(s->ctx, PT_ERR_INVALID_ARGUMENT, "material %llu: roughness outside [0,1]", (unsigned long long)i);
        // SPEC §5 DIELECTRIC with eta = ior or 1/ior in [2^-20, 2^20] (1/ior of a float in that range stays in it):
        //   eta*eta <= 2^40 is finite, so sin2t = eta*eta*(1 - cosi*cosi) is a number in [0, 2^40], never inf*0;
        //   past !(sin2t >= 1), sin2t <= 1 - 2^-24, so 1 - sin2t >= 2^-24 (exact for sin2t >= 1/2, rounded and >= 1/2 below),
        //   cost >= 2^-12 and ni*cost >= 2^-32 > 0: both Fresnel denominators are sums of a non-negative and a positive normal
        //   number, and rp and rs lie in [-1, 1];
        //   the refracted vector v = eta*d + (eta*cosi - cost)*n is finite (every term is below 2^21), and all that its
        //   normalisation needs beyond that is v != 0. The computed v need not be near unit length: cosi is a rounded, clamped
        //   cosine, so with eta near 2^20 and d a hair off -n the tangential part eta*d_t reaches about 2^8. But v's tangential
        //   part is eta*d_t alone (the n term has none), and its normal part is -cost + eta*(cosi - cos_true). At the ends of the
        //   range, where the roundings of v's components (up to eta*2^-23 = 2^-3) are largest, !(sin2t >= 1) forces cosi == 1
        //   (one float below 1 already gives sin2t = 2^17), hence sin2t = 0, cost = 1 and a normal part of -1 + eta*(1 - cos_true)
        //   in [-1, -1 + 2^-4]; towards the middle of the range the roundings shrink with eta. This is an argument for the ends,
        //   not a proof for every eta; tests/test_materials.py samples both ends, normal and grazing, on both sides.
        // An ior whose square overflows (<= 1e-20 or >= 1e20) gave sin2t = inf*0 = NaN at normal incidence and a NaN ray.
        if (mats[i].kind == PT_DIELECTRIC && !(mats[i].ior >= PT_IOR_MIN && mats[i].ior <= PT_IOR_MAX))
            return fail(s->ctx, PT_ERR_INVALID_ARGUMENT, "material %llu: ior outside [2^-20, 2^20]", (unsigned long long)i);
    }
    s->mats.assign(mats, mats + count);
    s->committed = false;
    return PT_OK;
}

pt_status pt_scene_set_triangle_uvs(pt_scene *s, const float *uv6, uint64_t count)
{
    if (!s) return fail(nullptr, PT_ERR_INVALID_ARGUMENT, "scene is NULL");
    if (count && !uv6) return fail(s->ctx, PT_ERR_INVALID_ARGUMENT, "pt_scene_set_triangle_uvs: uv6 is NULL");
    if (count >= (1ull << 28)) return fail(s->ctx, PT_ERR_UNSUPPORTED, "more than 2^28 triangles");
    for (uint64_t i = 0; i < count * 6; ++i)
        if (!(std::fabs(uv6[i]) <= 1048576.0f)) // (a NaN fails the comparison too)
            return fail(s->ctx, PT_ERR_INVALID_ARGUMENT, "pt_scene_set_triangle_uvs: float %llu is not finite or beyond 2^20", (unsigned long long)i);
    SceneTextures &T = s->textures;
    if (count) T.uvs.assign(uv6, uv6 + count * 6); else T.uvs.clear();
    T.have_uvs = count != 0; // (NULL, 0) and (non-NULL, 0) both leave a scene without UVs
    s->committed = false;
    return PT_OK;
}

pt_status pt_scene_set_texture(pt_scene *s, uint32_t index, const float *rgb, uint32_t width, uint32_t height, uint32_t flags)
{
    if (!s) return fail(nullptr, PT_ERR_INVALID_ARGUMENT, "scene is NULL");
    pt_context *c = s->ctx;
    if (index >= PT_MAX_TEXTURES) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_scene_set_texture: index %u, the limit is PT_MAX_TEXTURES = %u", index, PT_MAX_TEXTURES);
    SceneTextures::Texture &T = s->textures.tex[index];
    if (!rgb && width == 0 && height == 0) {
        if (flags) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_scene_set_texture: flags 0x%x with nothing to set", flags);
        T = SceneTextures::Texture{}; s->committed = false;
        return PT_OK;
    }
    if (!rgb) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_scene_set_texture: rgb is NULL");
    if (width < 1 || width > 4096 || height < 1 || height > 4096) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_scene_set_texture: %u x %u texels, each side must be in [1, 4096]", width, height);
    if (flags & ~(uint32_t)PT_TEXTURE_NEAREST) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_scene_set_texture: unknown flag bits 0x%x", flags & ~(uint32_t)PT_TEXTURE_NEAREST);
    const size_t n = (size_t)width * height * 3;
    for (size_t i = 0; i < n; ++i)
        if (!(std::isfinite(rgb[i]) && rgb[i] >= 0.f)) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_scene_set_texture: component %llu is not finite and >= 0", (unsigned long long)i);
    T.rgb.assign(rgb, rgb + n); T.width = width; T.height = height; T.flags = flags;
    s->committed = false;
    return PT_OK;
}

pt_status pt_scene_set_material_textures(pt_scene *s, const uint32_t *texture_of_material, uint64_t count)
{
    if (!s) return fail(nullptr, PT_ERR_INVALID_ARGUMENT, "scene is NULL");
    if (count && !texture_of_material) return fail(s->ctx, PT_ERR_INVALID_ARGUMENT, "pt_scene_set_material_textures: texture_of_material is NULL");
    for (uint64_t i = 0; i < count; ++i)
        if (texture_of_material[i] != PT_NO_TEXTURE && texture_of_material[i] >= PT_MAX_TEXTURES)
            return fail(s->ctx, PT_ERR_INVALID_ARGUMENT, "pt_scene_set_material_textures: material %llu: texture index %u, the limit is PT_MAX_TEXTURES = %u", (unsigned long long)i, texture_of_material[i], PT_MAX_TEXTURES);
    SceneTextures &T = s->textures;
    if (count) T.of_material.assign(texture_of_material, texture_of_material + count); else T.of_material.clear();
    T.have_binding = count != 0;
    s->committed = false;
    return PT_OK;
}

pt_status pt_scene_texture_info(const pt_scene *s, uint32_t index, pt_texture_info *out)
{
    if (!s || !out) return fail(s ? s->ctx : nullptr, PT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (index >= PT_MAX_TEXTURES) return fail(s->ctx, PT_ERR_INVALID_ARGUMENT, "pt_scene_texture_info: index %u, the limit is PT_MAX_TEXTURES = %u", index, PT_MAX_TEXTURES);
    const SceneTextures::Texture &T = s->textures.tex[index];
    std::memset(out, 0, sizeof *out);
    out->width = T.width; out->height = T.height; out->flags = T.flags;
    out->materials = T.width ? s->textures.bound_materials(index) : 0u;
    out->device_bytes = s->committed ? s->textures.device_bytes(index) : 0u;
    return PT_OK;
}

pt_status pt_scene_set_camera(pt_scene *s, const pt_camera *cam)
{
    if (!s || !cam) return fail(s ? s->ctx : nullptr, PT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!finite3(cam->origin) || !finite3(cam->forward) || !finite3(cam->right) || !finite3(cam->up) ||
        !std::isfinite(cam->scale) || !std::isfinite(cam->cx) || !std::isfinite(cam->cy))
        return fail(s->ctx, PT_ERR_INVALID_ARGUMENT, "camera has a non-finite field");
    s->cam = *cam; s->have_cam = true;
    if (s->committed) s->ds.cam = *cam; // camera changes do not need a re-commit
    return PT_OK;
}

pt_status pt_scene_set_sky(pt_scene *s, const float rgb[3])
{
    if (!s || !rgb) return fail(s ? s->ctx : nullptr, PT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!finite3(rgb)) return fail(s->ctx, PT_ERR_INVALID_ARGUMENT, "sky is not finite");
    for (int k = 0; k < 3; ++k) { s->sky[k] = rgb[k]; s->ds.sky[k] = rgb[k]; }
    return PT_OK;
}

pt_status pt_scene_set_lens(pt_scene *s, const pt_lens *lens)
{
    if (!s) return fail(nullptr, PT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!lens) { s->lens = pt_lens{}; return PT_OK; }
    if (!(std::isfinite(lens->radius) && lens->radius >= 0.f)) return fail(s->ctx, PT_ERR_INVALID_ARGUMENT, "pt_scene_set_lens: radius must be finite and >= 0");
    if (!(std::isfinite(lens->focus_distance) && lens->focus_distance > 0.f)) return fail(s->ctx, PT_ERR_INVALID_ARGUMENT, "pt_scene_set_lens: focus_distance must be finite and > 0");
    if (lens->flags) return fail(s->ctx, PT_ERR_INVALID_ARGUMENT, "pt_scene_set_lens: unknown flag bits 0x%x", lens->flags);
    s->lens = pt_lens{}; s->lens.radius = lens->radius; s->lens.focus_distance = lens->focus_distance;
    return PT_OK;
}

pt_status pt_scene_get_lens(const pt_scene *s, pt_lens *out)
{
    if (!s || !out) return fail(s ? s->ctx : nullptr, PT_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = s->lens;
    return PT_OK;
}

// ---- pt_scene_commit's phases, in the order they run. Each ends with a lap of the commit's clock.

// Check: the builder flag, the layout (bvh_width leaves as one of PT_BVH_WIDTH_2 .. _8O), the camera and every material id
static pt_status check_commit(const pt_scene *s, uint32_t &bvh_width, bool &lbvh)
{
    pt_context *c = s->ctx;
    lbvh = (bvh_width & PT_BVH_BUILD_LBVH) != 0; // hierarchy built on the GPU instead of the host SAH builder
    bvh_width &= ~(uint32_t)PT_BVH_BUILD_LBVH;
    if (lbvh && !c) return fail(c, PT_ERR_UNSUPPORTED, "PT_BVH_BUILD_LBVH needs a device context (detached scenes use the host builder)");
    // default layout: BVH4Q; scenes of up to ~200 triangles get BVH2 with float boxes — their whole tree is a handful of L1-resident
    // lines, memory does not count and the 2-wide visit is the cheapest in ALU. ms per 1080p / 64 spp frame, BVH8Q | BVH4Q | BVH4 | BVH2
    // (tools/exp_layouts.py): Cornell (12 triangles) 8.30 | 9.07 | 8.60 | 8.32, Cornell+glass+metal 9.82 | 11.34 | 9.82 | 9.18, walls of
    // 42 triangles 17.7 | 12.2 | 11.4 | 11.4, of 162: 18.7 | 14.2 | 13.4 | 12.7, of 252: - | 13.0 | 13.7 | 13.4, of 1002: 20.2 | 14.2 | 16.5 |
    // 15.0; soups of 100 / 400: - | 2.11 / 2.68 | 2.24 / 2.82 | 2.21 / 2.87. (Round 1 gave everything up to 256 triangles BVH8Q, on the
    // strength of the 12-triangle box alone, where it is one node.)
    if (bvh_width == PT_BVH_WIDTH_DEFAULT) bvh_width = s->tri_mat.size() <= 192 ? PT_BVH_WIDTH_2 : PT_BVH_WIDTH_4Q;
    if (bvh_width != PT_BVH_WIDTH_2 && bvh_width != PT_BVH_WIDTH_4 && bvh_width != PT_BVH_WIDTH_4Q && bvh_width != PT_BVH_WIDTH_8Q && bvh_width != PT_BVH_WIDTH_8O)
        return fail(c, PT_ERR_INVALID_ARGUMENT, "bvh_width must be one of PT_BVH_WIDTH_* (0, 2, 4, 68, 72, 73)");
    if (!s->have_cam) return fail(c, PT_ERR_INVALID_ARGUMENT, "no camera set");
    const uint32_t nt = (uint32_t)s->tri_mat.size(), ns = (uint32_t)s->sph_mat.size(), nm = (uint32_t)s->mats.size();
    if ((nt || ns) && nm == 0) return fail(c, PT_ERR_INVALID_ARGUMENT, "primitives but no materials");
    for (uint32_t i = 0; i < nt; ++i) if (s->tri_mat[i] >= nm) return fail(c, PT_ERR_INVALID_ARGUMENT, "triangle %u: material id %u >= %u", i, s->tri_mat[i], nm);
    for (uint32_t i = 0; i < ns; ++i) if (s->sph_mat[i] >= nm) return fail(c, PT_ERR_INVALID_ARGUMENT, "sphere %u: material id %u >= %u", i, s->sph_mat[i], nm);
    return s->textures.check(c, nt, nm); // docs/SPEC.md §13: the UV count, the binding's count and what it names
}

// Build tree: the hierarchy and its blob from the scene's current vertices, by one of three builders; the tree owner adopts the blob
// (and quantises a host-built one where the layout wants it). Only the first builder leaves the blob on the device alone.
static pt_status build_tree(pt_scene *s, uint32_t bvh_width, bool lbvh, CommitClock &clock)
{
    pt_context *c = s->ctx;
    const float *verts = nullptr;
    pt_status st = s->verts.host(c, verts); // updated since the last commit: build from the current vertices
    if (st != PT_OK) return st;
    const uint32_t nt = (uint32_t)s->tri_mat.size();
    const bool oct = bvh_width == PT_BVH_WIDTH_8O;
    const uint32_t fan = layout_fan(bvh_width);
    // the default layout is also packed on the device: nodes and triangle records are born in device memory
    const bool on_device = lbvh && nt >= 2 && bvh_width == PT_BVH_WIDTH_4Q;
    DeviceBlob4Q db; BvhBlob blob;
    if (on_device) {
        HIP_TRY(c, hipSetDevice(context_device(c)));
        HIP_TRY(c, build_lbvh_blob4q_device(context_stream(c), verts, s->tri_mat.data(), nt, db));
    } else if (lbvh && nt >= 2) {
        HIP_TRY(c, hipSetDevice(context_device(c)));
        BinaryBvh bt;
        HIP_TRY(c, build_lbvh_device(context_stream(c), verts, nt, bt));
        build_bvh_from_binary(bt, verts, s->tri_mat.data(), nt, fan, blob, oct);
    } else build_bvh(verts, s->tri_mat.data(), nt, fan, blob, oct);
    clock.lap("hierarchy + blob");
    const uint32_t depth = on_device ? db.max_depth : blob.max_depth;
    if (depth > 90) return fail(c, PT_ERR_INTERNAL, "BVH depth %u exceeds the supported 90", depth);
    if (on_device) s->tree.adopt(std::move(db), nt);
    else s->tree.adopt(std::move(blob), bvh_width);
    clock.lap("quantise");
    return PT_OK;
}

// Upload primitives: the spheres, their {material, 1/r} and the materials
static pt_status upload_primitives(pt_scene *s, CommitClock &clock)
{
    pt_context *c = s->ctx;
    const uint32_t ns = (uint32_t)s->sph_mat.size(), nm = (uint32_t)s->mats.size();
    HIP_TRY(c, s->d_spheres.ensure((ns + 3u) & ~3u)); // the kernels read the list four spheres (one 64-byte scalar load) at a time
    HIP_TRY(c, s->d_sph_mat.ensure(ns));
    HIP_TRY(c, s->d_mats.ensure((size_t)nm * 3));
    if (ns) {
        HIP_TRY(c, hipMemcpy(s->d_spheres.p, s->spheres.data(), (size_t)ns * 16, hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(s->d_sph_mat.p, sphere_mats(s->sph_mat.data(), s->spheres.data(), ns).data(), (size_t)ns * sizeof(uint2), hipMemcpyHostToDevice));
    }
    if (nm) HIP_TRY(c, hipMemcpy(s->d_mats.p, s->mats.data(), (size_t)nm * sizeof(pt_material), hipMemcpyHostToDevice));
    clock.lap("upload nodes + rest");
    return PT_OK;
}

// Light table of next-event estimation (docs/SPEC.md §7): the candidates, where their pa lives in the blob order, the table
static pt_status light_table(pt_scene *s, CommitClock &clock)
{
    pt_context *c = s->ctx;
    const uint32_t nt = (uint32_t)s->tri_mat.size(), nbt = s->tree.n_tris;
    s->light_cand.clear(); s->cand_blob.clear(); s->pa_span.clear(); s->cand_lo = 0; s->n_lights = 0;
    s->light_w.clear(); s->light_area.clear(); s->light_rec.clear(); s->light_blob.clear(); s->n_sph_lights = 0; s->jpa_zeroed = false;
    for (uint32_t i = 0; i < nt; ++i) {
        const float *e = s->mats[s->tri_mat[i]].emission;
        if (e[0] != 0.f || e[1] != 0.f || e[2] != 0.f) s->light_cand.push_back(i);
    }
    HIP_TRY(c, s->d_pa.ensure(std::max<size_t>(nbt, 1)));
    HIP_TRY(c, hipMemset(s->d_pa.p, 0, std::max<size_t>(nbt, 1) * sizeof(float)));
    if (!s->light_cand.empty()) {
        std::vector<uint32_t> blob_of(nt), ids;
        pt_status st = s->tree.ids(c, ids);
        if (st != PT_OK) return st;
        for (uint32_t j = 0; j < nbt; ++j) blob_of[ids[j]] = j;
        uint32_t hi = 0; s->cand_lo = nbt;
        for (const uint32_t id : s->light_cand) {
            const uint32_t b = blob_of[id];
            s->cand_blob.push_back(b); s->cand_lo = std::min(s->cand_lo, b); hi = std::max(hi, b);
        }
        s->pa_span.assign(hi - s->cand_lo + 1u, 0.0f);
        const float *verts = nullptr;
        if ((st = s->verts.host(c, verts)) != PT_OK || (st = build_lights(c, s, verts, 0)) != PT_OK) return st;
    } else { // no triangle can be a light: the joint table is the spheres'
        const pt_status st = build_sphere_lights(c, s);
        if (st != PT_OK) return st;
    }
    clock.lap("light table");
    return PT_OK;
}

// Publish: what the kernels see of the scene
static void publish_scene(pt_scene *s)
{
    DeviceScene &d = s->ds;
    d.nodes = s->tree.d_nodes.p; d.tris = s->tree.d_tris.p; d.spheres = s->d_spheres.p; d.sph_mat = s->d_sph_mat.p; d.mats = s->d_mats.p;
    d.n_nodes = s->tree.n_nodes; d.n_tris = (uint32_t)s->tri_mat.size(); d.n_spheres = (uint32_t)s->sph_mat.size(); d.n_mats = (uint32_t)s->mats.size();
    for (int k = 0; k < 3; ++k) d.sky[k] = s->sky[k];
    d.bvh_width = s->tree.layout;
    d.cam = s->cam;
    s->has_specular = false;
    for (const pt_material &m : s->mats) if (m.kind != PT_LAMBERT) s->has_specular = true;
    s->committed = true;
}

pt_status pt_scene_commit(pt_scene *s, uint32_t bvh_width)
{
    if (!s) return fail(nullptr, PT_ERR_INVALID_ARGUMENT, "scene is NULL");
    bool lbvh = false;
    pt_status st = check_commit(s, bvh_width, lbvh);
    if (st != PT_OK) return st;
    CommitClock clock;
    s->serial = next_scene_serial(); s->updates = 0; // a new tree: nothing recorded from the old one describes it
    s->cache.invalidate(); // level lists, guide index and what earlier frames measured belong to the tree this commit replaces
    if ((st = build_tree(s, bvh_width, lbvh, clock)) != PT_OK) return st;
    if (!s->ctx) { // detached scene: host-side blob only
        if ((st = s->textures.commit(nullptr, s->tri_mat, s->tree)) != PT_OK) return st;
        s->committed = true; return PT_OK;
    }
    if ((st = s->tree.upload(s->ctx, clock)) != PT_OK || (st = upload_primitives(s, clock)) != PT_OK || (st = light_table(s, clock)) != PT_OK) return st;
    // docs/SPEC.md §13: behind the tree, which it reads (the blob order) and does not touch — the same tree and blob with and without textures
    if ((st = s->textures.commit(s->ctx, s->tri_mat, s->tree)) != PT_OK) return st;
    clock.lap("textures");
    // the root's boxes as the device holds them, whichever builder made them (frame.cpp scene_pixels)
    HIP_TRY(s->ctx, s->tree.fetch_root(context_stream(s->ctx))); HIP_TRY(s->ctx, hipStreamSynchronize(context_stream(s->ctx)));
    s->tree.root_fetched();
    publish_scene(s);
    return PT_OK;
}

pt_status pt_scene_bvh_info(const pt_scene *s, pt_bvh_info *o)
{
    if (!s || !o) return fail(s ? s->ctx : nullptr, PT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!s->committed) return fail(s->ctx, PT_ERR_NOT_COMMITTED, "scene not committed");
    std::memset(o, 0, sizeof *o);
    const CommittedTree &t = s->tree;
    o->width = t.layout; o->n_nodes = t.n_nodes; o->n_tris = t.n_tris;
    o->max_depth = t.max_depth;
    o->node_bytes = t.node_bytes;
    o->tri_bytes = (uint64_t)t.n_tris * sizeof(BvhTri);
    o->build_ms = t.build_ms; o->sah_cost = t.sah_cost;
    o->stack_need = t.stack_need;
    return PT_OK;
}

pt_status pt_scene_bvh_read(const pt_scene *s, void *nodes, uint64_t node_bytes, void *tris48, uint64_t tri_bytes)
{
    if (!s) return fail(nullptr, PT_ERR_INVALID_ARGUMENT, "scene is NULL");
    if (!s->committed) return fail(s->ctx, PT_ERR_NOT_COMMITTED, "scene not committed");
    const void *img_nodes = nullptr; const BvhTri *img_tris = nullptr;
    const pt_status st = s->tree.host_image(s->ctx, img_nodes, img_tris);
    if (st != PT_OK) return st;
    const uint64_t nb = s->tree.node_bytes, tb = (uint64_t)s->tree.n_tris * sizeof(BvhTri);
    if (node_bytes < nb || tri_bytes < tb || (nb && !nodes) || (tb && !tris48)) return fail(s->ctx, PT_ERR_INVALID_ARGUMENT, "buffers too small: need %llu + %llu bytes", (unsigned long long)nb, (unsigned long long)tb);
    if (nb) std::memcpy(nodes, img_nodes, nb);
    if (tb) std::memcpy(tris48, img_tris, tb);
    return PT_OK;
}

// ------------------------------------------------------------------------------------------------ geometry updates (docs/SPEC.md §4.3)

// The first update after a commit: level lists from the tree's refs (in device node order) and the
// scratch the passes use. Sizes are those of the committed tree, which an update never changes.
static pt_status prepare_refit(pt_scene *s)
{
    pt_context *c = s->ctx;
    auto &R = s->cache.refit;
    const uint32_t nn = s->tree.n_nodes, fan = s->tree.fan, nbt = s->tree.n_tris;
    for (auto &e : R.ev) HIP_TRY(c, e.create());
    std::vector<int32_t> refs;
    const pt_status st = s->tree.refs(c, refs);
    if (st != PT_OK) return st;
    std::vector<uint32_t> list;
    if (!refit_levels(refs.data(), nn, fan, nbt, list, R.level_off)) return fail(c, PT_ERR_INTERNAL, "pt_scene_update_triangles: the committed tree's refs do not form a tree");
    HIP_TRY(c, R.list.ensure(list.size()));
    if (!list.empty()) HIP_TRY(c, hipMemcpy(R.list.p, list.data(), list.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(c, R.tbox.ensure((size_t)nbt * 6)); HIP_TRY(c, R.nbox.ensure((size_t)nn * 6)); HIP_TRY(c, R.carea.ensure((size_t)nn * fan));
    HIP_TRY(c, s->verts.reserve_device());
    HIP_TRY(c, R.sah.ensure(refit_sah_blocks(nn) + 1u)); HIP_TRY(c, R.flag.ensure(1));
    R.ready = true;
    return PT_OK;
}

static pt_status update_triangles(pt_scene *s, const void *verts9, uint64_t count, uint32_t flags, pt_stats *stats)
{
    if (!s) return fail(nullptr, PT_ERR_INVALID_ARGUMENT, "pt_scene_update_triangles: scene is NULL");
    pt_context *c = s->ctx;
    if (flags & ~(uint32_t)PT_UPDATE_HOST_MEMORY) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_scene_update_triangles: unknown flag bits 0x%x", flags & ~(uint32_t)PT_UPDATE_HOST_MEMORY);
    if (!s->committed) return fail(c, PT_ERR_NOT_COMMITTED, "pt_scene_update_triangles: scene not committed");
    const uint64_t nt = s->tri_mat.size();
    if (count != nt) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_scene_update_triangles: count %llu, the scene was committed with %llu triangles", (unsigned long long)count, (unsigned long long)nt);
    if (count && !verts9) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_scene_update_triangles: verts9 is NULL");
    const bool host = (flags & PT_UPDATE_HOST_MEMORY) != 0;
    if (host) {
        const float *v = (const float *)verts9;
        for (uint64_t i = 0; i < count * 9; ++i)
            if (!std::isfinite(v[i])) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_scene_update_triangles: non-finite vertex coordinate at float %llu", (unsigned long long)i);
    }
    if (!c) return fail(c, PT_ERR_UNSUPPORTED, "pt_scene_update_triangles: a detached scene has no device tree to refit (set the triangles and commit)");
    pt_stats out{};
    if (count == 0) { if (stats) *stats = out; return PT_OK; }
    HIP_TRY(c, hipSetDevice(context_device(c)));
    pt_status st;
    if (!host) {
        if ((uintptr_t)verts9 & 3u) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_scene_update_triangles: verts9 must be 4-byte aligned");
        if ((st = check_device_array(c, verts9, count * 36u, "verts9", "pt_scene_update_triangles", "PT_UPDATE_HOST_MEMORY")) != PT_OK) return st;
    }
    auto &R = s->cache.refit;
    if (!R.ready && (st = prepare_refit(s)) != PT_OK) return st;
    hipStream_t q = context_stream(c);
    const CommittedTree &tree = s->tree;
    float *v = s->verts.next(); // the buffer that does not hold the scene's current vertices
    if (host) HIP_TRY(c, hipMemcpyAsync(v, verts9, count * 36u, hipMemcpyHostToDevice, q));
    HIP_TRY(c, hipEventRecord(R.ev[0], q));
    float ms_check = 0.f;
    if (!host) { // the non-finite reduction runs (and copies the batch aside) before anything of the scene is written
        HIP_TRY(c, hipMemsetAsync(R.flag.p, 0, sizeof(uint32_t), q));
        HIP_TRY(c, launch_refit_stage(q, (const float *)verts9, v, count * 9u, R.flag.p));
        HIP_TRY(c, hipEventRecord(R.ev[1], q));
        uint32_t bad = 0;
        HIP_TRY(c, hipMemcpyAsync(&bad, R.flag.p, sizeof bad, hipMemcpyDeviceToHost, q));
        HIP_TRY(c, hipStreamSynchronize(q));
        if (bad) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_scene_update_triangles: non-finite vertex coordinate in the device array");
        HIP_TRY(c, hipEventElapsedTime(&ms_check, R.ev[0], R.ev[1]));
        HIP_TRY(c, hipEventRecord(R.ev[0], q));
    }
    const uint32_t layout = tree.layout;
    ++s->updates; // from here on the device records are rewritten (counted even if the update then fails)
    s->tree.bound_stale(); // ... and the root's boxes with them: read back below, behind the last pass
    HIP_TRY(c, launch_refit_tris(q, v, tree.d_tris.p, tree.n_tris, R.tbox.p));
    for (size_t l = 0; l + 1 < R.level_off.size(); ++l)
        HIP_TRY(c, launch_refit_level(q, layout, tree.d_nodes.p, R.list.p + R.level_off[l], R.level_off[l + 1] - R.level_off[l], R.tbox.p, R.nbox.p, R.carea.p));
    const uint32_t nb = refit_sah_blocks(tree.n_nodes);
    HIP_TRY(c, launch_refit_sah(q, layout, tree.d_nodes.p, tree.n_nodes, R.carea.p, R.nbox.p, R.sah.p, R.sah.p + nb));
    HIP_TRY(c, hipEventRecord(R.ev[2], q));
    double sah = 0.0;
    HIP_TRY(c, hipMemcpyAsync(&sah, R.sah.p + nb, sizeof sah, hipMemcpyDeviceToHost, q));
    HIP_TRY(c, s->tree.fetch_root(q));
    HIP_TRY(c, hipStreamSynchronize(q));
    s->tree.root_fetched();
    float ms = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms, R.ev[0], R.ev[2]));
    out.gpu_ms = (double)ms + ms_check;
    if (!s->pa_span.empty()) { // the light table from the new vertices of the candidates (same candidates: the materials stay)
        const uint32_t lo = s->light_cand.front(), hi = s->light_cand.back(); // in triangle order
        std::vector<float> span(host ? 0u : (size_t)(hi - lo + 1u) * 9u); // a device array: only the candidates' span comes back
        if (!host) HIP_TRY(c, hipMemcpy(span.data(), v + (size_t)lo * 9u, span.size() * sizeof(float), hipMemcpyDeviceToHost));
        if ((st = host ? build_lights(c, s, (const float *)verts9, 0) : build_lights(c, s, span.data(), lo)) != PT_OK) return st;
    }
    s->verts.next_is_current(); // all of the update has succeeded
    s->tree.device_rewritten((float)sah);
    if (stats) *stats = out;
    return PT_OK;
}

static pt_status update_spheres(pt_scene *s, const float *cxyzr, uint64_t count)
{
    if (!s) return fail(nullptr, PT_ERR_INVALID_ARGUMENT, "pt_scene_update_spheres: scene is NULL");
    pt_context *c = s->ctx;
    if (!s->committed) return fail(c, PT_ERR_NOT_COMMITTED, "pt_scene_update_spheres: scene not committed");
    const uint64_t ns = s->sph_mat.size();
    if (count != ns) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_scene_update_spheres: count %llu, the scene was committed with %llu spheres", (unsigned long long)count, (unsigned long long)ns);
    if (count && !cxyzr) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_scene_update_spheres: cxyzr is NULL");
    for (uint64_t i = 0; i < count; ++i)
        if (!sphere_ok(cxyzr + i * 4)) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_scene_update_spheres: sphere %llu: non-finite centre or radius <= 0", (unsigned long long)i);
    if (!c) return fail(c, PT_ERR_UNSUPPORTED, "pt_scene_update_spheres: a detached scene has no device copy to update (set the spheres and commit)");
    if (count == 0) return PT_OK;
    HIP_TRY(c, hipSetDevice(context_device(c)));
    const std::vector<uint2> mi = sphere_mats(s->sph_mat.data(), cxyzr, count);
    hipStream_t q = context_stream(c);
    ++s->updates; // from here on the device records are rewritten
    HIP_TRY(c, hipMemcpyAsync(s->d_spheres.p, cxyzr, count * 16u, hipMemcpyHostToDevice, q));
    HIP_TRY(c, hipMemcpyAsync(s->d_sph_mat.p, mi.data(), count * sizeof(uint2), hipMemcpyHostToDevice, q));
    HIP_TRY(c, hipStreamSynchronize(q));
    s->spheres.assign(cxyzr, cxyzr + count * 4);
    return build_sphere_lights(c, s); // §7.1: the sphere part of the joint table from the new centres and radii
}

pt_status pt_scene_update_triangles(pt_scene *s, const void *verts9, uint64_t count, uint32_t flags, pt_stats *stats)
{
    return drained_on_failure(s ? s->ctx : nullptr, [&] { return update_triangles(s, verts9, count, flags, stats); });
}

pt_status pt_scene_update_spheres(pt_scene *s, const float *cxyzr, uint64_t count)
{
    return drained_on_failure(s ? s->ctx : nullptr, [&] { return update_spheres(s, cxyzr, count); });
}

// scene.h: the GPU builder's binary tree, for the tests
pt_status pt_internal_lbvh_binary(pt_context *c, const float *verts9, uint64_t n, uint32_t *order, int32_t *left, int32_t *right,
                                  uint32_t *first, uint32_t *last, float *box6)
{
    if (!c || !verts9 || !order || !left || !right || !first || !last || !box6) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_internal_lbvh_binary: NULL argument");
    if (n < 2 || n >= (1ull << 28)) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_internal_lbvh_binary: %llu triangles, need 2 .. 2^28 - 1", (unsigned long long)n);
    for (uint64_t i = 0; i < n * 9; ++i)
        if (!std::isfinite(verts9[i])) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_internal_lbvh_binary: non-finite vertex coordinate at float %llu", (unsigned long long)i);
    return drained_on_failure(c, [&]() -> pt_status {
        HIP_TRY(c, hipSetDevice(context_device(c)));
        BinaryBvh bt;
        HIP_TRY(c, build_lbvh_device(context_stream(c), verts9, (uint32_t)n, bt));
        std::memcpy(order, bt.order.data(), n * 4);
        std::memcpy(left, bt.left.data(), (n - 1) * 4); std::memcpy(right, bt.right.data(), (n - 1) * 4);
        std::memcpy(first, bt.first.data(), (n - 1) * 4); std::memcpy(last, bt.last.data(), (n - 1) * 4);
        std::memcpy(box6, bt.box.data(), (n - 1) * 24);
        return PT_OK;
    });
}

} // extern "C"
