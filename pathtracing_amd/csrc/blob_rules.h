// blob_rules.h — the rules of the docs/SPEC.md §4.1 blob that more than one of its producers follows, stated once: the host SAH builder
// (bvh_build.cpp, scene.cpp), the GPU builder (lbvh.hip) and the refit (refit.hip) promise the same bytes for the same tree, and they get
// them by calling the same text. Plain C++ and device code both: bvh_build.cpp is compiled without HIP. Every operation has one
// spelling that both sides compile to the same IEEE result on the finite numbers the builders see (-ffp-contract=off, correctly
// rounded divide and sqrt): compiler builtins for fma, sqrt, floor, ceil, frexp and fabs, `<` and `?:` for min and max.
// The consumer (kernels.hip, pt_device.h) keeps its own decode; oracle/ and tests/ray_caster64.py restate the format as checkers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/ptrt.h"

#ifdef __HIP__
#define PT_HD __host__ __device__
#else
#define PT_HD
#endif

namespace ptrt {

// ---- constants and the leaf encoding
constexpr int32_t kEmptyRef = 0x7fffffff; // a child slot without a child
constexpr uint32_t kMaxLeaf = 4;          // triangles per leaf, at most
#ifndef PT_LBVH_CLUSTER
#define PT_LBVH_CLUSTER 32
#endif
constexpr uint32_t kClusterTris = PT_LBVH_CLUSTER; // the GPU builder's LBVH is cut into subtrees of at most this many triangles (1: every triangle a cluster)
static_assert(kClusterTris >= 1, "a cluster holds at least one triangle: there is no build without the SAH top storey");

PT_HD constexpr int32_t leaf_ref(uint32_t first, uint32_t count) { return (int32_t)~((first << 3) | (count - 1u)); } // records [first, first + count)
PT_HD constexpr uint32_t leaf_first(int32_t ref) { return (uint32_t)~ref >> 3; }
PT_HD constexpr uint32_t leaf_count(int32_t ref) { return ((uint32_t)~ref & 7u) + 1u; }

template <class T> PT_HD constexpr T rule_min(T a, T b) { return b < a ? b : a; }
template <class T> PT_HD constexpr T rule_max(T a, T b) { return a < b ? b : a; }

// ---- boxes
struct Box {
    float lo[3], hi[3];
    PT_HD static Box empty()
    {
        Box b;
        for (int k = 0; k < 3; ++k) { b.lo[k] = __builtin_inff(); b.hi[k] = -__builtin_inff(); }
        return b;
    }
    PT_HD static Box of(const float *p6) // lo xyz, hi xyz
    {
        Box b;
        for (int k = 0; k < 3; ++k) { b.lo[k] = p6[k]; b.hi[k] = p6[3 + k]; }
        return b;
    }
    PT_HD void grow(const Box &b) { for (int k = 0; k < 3; ++k) { lo[k] = rule_min(lo[k], b.lo[k]); hi[k] = rule_max(hi[k], b.hi[k]); } }
    PT_HD float area() const
    {
        const float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
        return (dx < 0.f) ? 0.f : 2.f * (dx * dy + dy * dz + dz * dx);
    }
};

PT_HD inline float pad_of(float c) { return 1e-6f * rule_max(1.0f, __builtin_fabsf(c)); }

// The padded leaf box of a triangle (nine floats). cent, if given: the centre of the unpadded box, what both builders sort by.
PT_HD inline Box tri_box(const float *p, float *cent = nullptr)
{
    Box b;
    for (int k = 0; k < 3; ++k) {
        const float lo = rule_min(p[k], rule_min(p[3 + k], p[6 + k])), hi = rule_max(p[k], rule_max(p[3 + k], p[6 + k]));
        b.lo[k] = lo - pad_of(lo); b.hi[k] = hi + pad_of(hi);
        if (cent) cent[k] = 0.5f * (lo + hi);
    }
    return b;
}

// ---- the 64-byte triangle record: v0 | id, e1 | mat, e2 | 0, normalize(cross(e1, e2)) | mat. Rows 0-2 are the blob's 48-byte triangle.
PT_HD inline float bits_as_float(uint32_t u) { return __builtin_bit_cast(float, u); }

// n = normalize(cross(e1, e2)) in exactly the op order of docs/SPEC.md §0 (fma, IEEE sqrt and divide), so the bits equal what the kernel
// would compute from e1, e2: a triangle record's shading row, a light's normal. Returns |cross(e1, e2)|^2.
PT_HD inline float shading_normal(const float *e1, const float *e2, float *n)
{
    const float cr[3] = { __builtin_fmaf(e1[1], e2[2], -(e1[2] * e2[1])), __builtin_fmaf(e1[2], e2[0], -(e1[0] * e2[2])), __builtin_fmaf(e1[0], e2[1], -(e1[1] * e2[0])) };
    const float dd = __builtin_fmaf(cr[2], cr[2], __builtin_fmaf(cr[1], cr[1], cr[0] * cr[0])), inv = 1.0f / __builtin_sqrtf(dd);
    for (int k = 0; k < 3; ++k) n[k] = cr[k] * inv;
    return dd;
}
PT_HD inline void tri_rows(const float *v, uint32_t id, uint32_t mat, float *r12) // rows 0-2
{
    for (int k = 0; k < 3; ++k) { r12[k] = v[k]; r12[4 + k] = v[3 + k] - v[k]; r12[8 + k] = v[6 + k] - v[k]; }
    r12[3] = bits_as_float(id); r12[7] = bits_as_float(mat); r12[11] = 0.f;
}
PT_HD inline void shading_row(const float *e1, const float *e2, uint32_t mat, float *r4) // row 3
{
    shading_normal(e1, e2, r4);
    r4[3] = bits_as_float(mat);
}
PT_HD inline void tri_record(const float *v, uint32_t id, uint32_t mat, float *r16)
{
    tri_rows(v, id, mat, r16);
    shading_row(r16 + 4, r16 + 8, mat, r16 + 12);
}

// ---- node layouts by PT_BVH_WIDTH_* code: children per node, quantised or f32 slots, bytes per node, where child c's ref sits
PT_HD constexpr uint32_t layout_fan(uint32_t L) { return L == PT_BVH_WIDTH_2 ? 2u : (L == PT_BVH_WIDTH_8Q || L == PT_BVH_WIDTH_8O) ? 8u : 4u; }
PT_HD constexpr bool layout_quantised(uint32_t L) { return L == PT_BVH_WIDTH_4Q || L == PT_BVH_WIDTH_8Q || L == PT_BVH_WIDTH_8O; }
PT_HD constexpr uint32_t layout_node_bytes(uint32_t L) { return layout_quantised(L) ? (layout_fan(L) == 4u ? 64u : 128u) : 32u * layout_fan(L); }
PT_HD constexpr uint32_t layout_ref_at(uint32_t L, uint32_t c) { return layout_quantised(L) ? 16u + 4u * c : 32u * c + 12u; } // quantised: i32 refs from byte 16; f32: row 0 .w of slot c
template <int L> struct Layout {
    static constexpr int N = (int)layout_fan(L);
    static constexpr bool Q = layout_quantised(L);
    static constexpr size_t kStride = layout_node_bytes(L);
    PT_HD static int32_t ref(const uint8_t *nd, int c) { return *reinterpret_cast<const int32_t *>(nd + layout_ref_at(L, (uint32_t)c)); }
};

// ---- the quantiser of layouts 68, 72, 73
PT_HD inline float quant_scale_of(uint32_t e) { return bits_as_float(e << 23); }

// One node of N = 4 (64 bytes) or N = 8 (128 bytes) children. Per axis a power-of-two grid from the children's union; every decoded box
// encloses its float box, checked with the traversal's own expression fma((float)q, scale, origin). Writes origin | exponents (words
// 0-3) and the quantised coordinates (from byte 16 + 4N: qlo_x, qlo_y, qlo_z, qhi_x, qhi_y, qhi_z, N bytes each, child c in byte c);
// N = 4 also zeroes the pad words 14-15. The refs (words 4 .. 3 + N) are the caller's. B: any type with float lo[3], hi[3].
template <int N, class B>
PT_HD inline void quantize_node(const B *box, const bool *used, uint32_t *w)
{
    static_assert(N == 4 || N == 8, "BVH4Q / BVH8Q nodes");
    constexpr int kW = N / 4; // u32 words per coordinate group
    float org[3]; uint32_t ex[3];
    uint32_t qlo[3][kW], qhi[3][kW];
    for (int a = 0; a < 3; ++a) {
        float lo = __builtin_inff(), hi = -__builtin_inff();
        for (int c = 0; c < N; ++c) if (used[c]) { lo = rule_min(lo, box[c].lo[a]); hi = rule_max(hi, box[c].hi[a]); }
        if (!(lo <= hi)) lo = hi = 0.f; // node without children (cannot happen for a built tree)
        org[a] = lo;
        int e = 1;
        { // smallest power of two with 255 * scale >= extent
            const float ext = hi - lo;
            int ee; const float m = __builtin_frexpf(ext / 255.0f, &ee); // ext / 255 = m * 2^ee, m in [0.5, 1)
            e = (ext > 0.f) ? ee + 127 - (m == 0.5f ? 1 : 0) : 1;
            e = rule_min(rule_max(e, 1), 254);
        }
        for (;;) { // quantise; widen the grid if a coordinate does not fit in 8 bits
            const float sc = quant_scale_of((uint32_t)e);
            bool ok = true;
            uint32_t pl[kW], ph[kW];
            for (int k = 0; k < kW; ++k) pl[k] = ph[k] = 0u;
            for (int c = 0; c < N && ok; ++c) {
                if (!used[c]) continue;
                int ql = (int)__builtin_floorf((box[c].lo[a] - lo) / sc), qh = (int)__builtin_ceilf((box[c].hi[a] - lo) / sc);
                ql = rule_min(rule_max(ql, 0), 255); qh = rule_min(rule_max(qh, 0), 255);
                while (ql > 0 && !(__builtin_fmaf((float)ql, sc, lo) <= box[c].lo[a])) --ql;
                while (qh < 255 && !(__builtin_fmaf((float)qh, sc, lo) >= box[c].hi[a])) ++qh;
                if (!(__builtin_fmaf((float)ql, sc, lo) <= box[c].lo[a]) || !(__builtin_fmaf((float)qh, sc, lo) >= box[c].hi[a])) { ok = false; break; }
                pl[c / 4] |= (uint32_t)ql << (8 * (c % 4)); ph[c / 4] |= (uint32_t)qh << (8 * (c % 4));
            }
            if (ok || e >= 254) { for (int k = 0; k < kW; ++k) { qlo[a][k] = pl[k]; qhi[a][k] = ph[k]; } break; }
            ++e;
        }
        ex[a] = (uint32_t)e;
    }
    w[0] = __builtin_bit_cast(uint32_t, org[0]); w[1] = __builtin_bit_cast(uint32_t, org[1]); w[2] = __builtin_bit_cast(uint32_t, org[2]);
    w[3] = ex[0] | (ex[1] << 8) | (ex[2] << 16);
    constexpr int q0 = 4 + N; // first word of the quantised coordinates
    for (int a = 0; a < 3; ++a)
        for (int k = 0; k < kW; ++k) { w[q0 + kW * a + k] = qlo[a][k]; w[q0 + kW * (3 + a) + k] = qhi[a][k]; }
    if (N == 4) { w[14] = 0u; w[15] = 0u; }
}

// ---- SAH cost of a blob: the sum over child slots of this term, in double (pt_bvh_info.sah_cost is the sum rounded to f32)
PT_HD inline float sah_root_area(const Box &root) { return rule_max(root.area(), 1e-30f); }
PT_HD inline double sah_child_term(float area, float root_area, int32_t ref) // area / root area (an f32 quotient), times the triangle count for a leaf
{
    return (double)(area / root_area) * (double)(ref < 0 ? leaf_count(ref) : 1u);
}

// ---- packing a binary LBVH (lbvh.hip on the device for layout 68, bvh_build.cpp build_bvh_from_binary for the others)
// The leaf rule: a subtree of at most kMaxLeaf triangles becomes one leaf unless splitting it into its two children lowers the SAH cost.
PT_HD inline bool lbvh_leaf(uint32_t count, float area, uint32_t lcount, float larea, uint32_t rcount, float rarea)
{
    if (count > kMaxLeaf) return false;
    float split = 0.f;
    split += larea * (float)lcount;
    split += rarea * (float)rcount;
    return !(split < area * (float)count);
}

// ---- depth and worst-case traversal-stack need of one node: give it every child slot's ref, with the figures of the nodes below it
struct DepthNeed {
    uint32_t used = 0, dmax = 1, nmax = 0; // children, the largest inner child's depth and need
    PT_HD void child(int32_t ref, const uint32_t *depth_of, const uint32_t *need_of)
    {
        if (ref == kEmptyRef) return;
        ++used;
        if (ref >= 0) { dmax = rule_max(dmax, depth_of[ref]); nmax = rule_max(nmax, need_of[ref]); }
    }
    PT_HD uint32_t depth() const { return dmax + 1; }
    PT_HD uint32_t need() const { return (used ? used - 1 : 0) + nmax; } // all children pushed but the one entered, then the deepest of them
};

} // namespace ptrt
