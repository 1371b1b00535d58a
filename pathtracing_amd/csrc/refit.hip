// refit.hip — pt_scene_update_triangles on the device (docs/SPEC.md §4.3). The committed tree keeps its topology, its leaf assignment
// and its memory order; only the numbers change:
//   k_refit_stage : device input -> the scene's spare vertex buffer, with a flag for any non-finite coordinate (read before anything of
//                   the scene is written)
//   k_refit_tris  : every triangle record rewritten from the new vertices (lbvh.hip k_tri_records' arithmetic), and its padded box
//   k_refit_level : one launch per tree level, deepest first: a node's child boxes from its leaves' triangle boxes and its inner children's
//                   unions, written as f32 slots or re-quantised (quantize_node.h, the GPU builder's own quantiser)
//   k_refit_sah   : the builder's SAH cost of the new boxes, reduced in a fixed order
// Every box is an exact union (min / max) of padded triangle boxes made from the input vertices, which is what every builder puts in
// the blob, so the refitted blob is a blob a builder could have emitted for the new vertices: it renders that commit's picture (§4.1).
#include <hip/hip_runtime.h>
#include "refit.h"
#include "quantize_node.h"
#include "../../include/ptrt.h"

namespace ptrt {
namespace {

constexpr int32_t kEmptyRef = 0x7fffffff;
constexpr uint32_t kBlock = 256;

struct RBox { float lo[3], hi[3]; };
__device__ __forceinline__ float pad_of(float c) { return 1e-6f * fmaxf(1.0f, fabsf(c)); } // bvh_build.cpp tri_box, lbvh.hip k_tri_boxes
__device__ __forceinline__ float area_of(const RBox &b)                                     // bvh_build.cpp Box::area
{
    const float dx = b.hi[0] - b.lo[0], dy = b.hi[1] - b.lo[1], dz = b.hi[2] - b.lo[2];
    return dx < 0.f ? 0.f : 2.f * (dx * dy + dy * dz + dz * dx);
}
__device__ __forceinline__ void set_empty(RBox &b) { for (int k = 0; k < 3; ++k) { b.lo[k] = __builtin_inff(); b.hi[k] = -__builtin_inff(); } }
__device__ __forceinline__ void grow(RBox &b, const float *p6)
{
    for (int k = 0; k < 3; ++k) { b.lo[k] = fminf(b.lo[k], p6[k]); b.hi[k] = fmaxf(b.hi[k], p6[3 + k]); }
}

__global__ void __launch_bounds__(kBlock) k_refit_stage(const float *__restrict__ in, float *__restrict__ out, uint64_t n, uint32_t *__restrict__ bad)
{
    bool finite = true;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        const float v = in[i];
        out[i] = v;
        finite = finite && (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u;
    }
    if (!finite) atomicOr(bad, 1u); // only a rejected batch pays for atomics
}

__global__ void __launch_bounds__(kBlock) k_refit_tris(const float *__restrict__ verts, float4 *__restrict__ rec, uint32_t n, float *__restrict__ tbox)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    const float4 r0 = rec[(size_t)j * 4], r1 = rec[(size_t)j * 4 + 1];
    const uint32_t id = __float_as_uint(r0.w);
    const float *v = verts + (size_t)id * 9;
    const float p[9] = { v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8] };
    const float a[3] = { p[3] - p[0], p[4] - p[1], p[5] - p[2] }, b[3] = { p[6] - p[0], p[7] - p[1], p[8] - p[2] };
    const float cx = __builtin_fmaf(a[1], b[2], -(a[2] * b[1])), cy = __builtin_fmaf(a[2], b[0], -(a[0] * b[2])), cz = __builtin_fmaf(a[0], b[1], -(a[1] * b[0]));
    const float inv = 1.0f / __builtin_sqrtf(__builtin_fmaf(cz, cz, __builtin_fmaf(cy, cy, cx * cx)));
    rec[(size_t)j * 4 + 0] = make_float4(p[0], p[1], p[2], r0.w);
    rec[(size_t)j * 4 + 1] = make_float4(a[0], a[1], a[2], r1.w);
    rec[(size_t)j * 4 + 2] = make_float4(b[0], b[1], b[2], 0.f);
    rec[(size_t)j * 4 + 3] = make_float4(cx * inv, cy * inv, cz * inv, r1.w);
    for (int k = 0; k < 3; ++k) { // the padded leaf box of docs/SPEC.md §4.1, from the input vertices
        const float lo = fminf(p[k], fminf(p[3 + k], p[6 + k])), hi = fmaxf(p[k], fmaxf(p[3 + k], p[6 + k]));
        tbox[(size_t)j * 6 + k] = lo - pad_of(lo);
        tbox[(size_t)j * 6 + 3 + k] = hi + pad_of(hi);
    }
}

// node geometry of a layout: children per node, quantised or f32 slots, bytes per node
template <int L> struct Layout {
    static constexpr int N = L == PT_BVH_WIDTH_2 ? 2 : (L == PT_BVH_WIDTH_4 || L == PT_BVH_WIDTH_4Q) ? 4 : 8;
    static constexpr bool Q = L == PT_BVH_WIDTH_4Q || L == PT_BVH_WIDTH_8Q || L == PT_BVH_WIDTH_8O;
    static constexpr size_t kStride = Q ? (N == 4 ? 64 : 128) : 32 * N;
    __device__ static int32_t ref(const uint8_t *nd, int c) // quantised: i32 refs at byte 16; f32: row 0 .w of slot c
    {
        return Q ? reinterpret_cast<const int32_t *>(nd + 16)[c] : reinterpret_cast<const int32_t *>(nd + 32 * c)[3];
    }
};

template <int L>
__global__ void __launch_bounds__(kBlock) k_refit_level(uint8_t *__restrict__ nodes, const uint32_t *__restrict__ list, uint32_t count,
                                                        const float *__restrict__ tbox, float *__restrict__ nbox, float *__restrict__ carea)
{
    using Lay = Layout<L>;
    constexpr int N = Lay::N;
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    if (q >= count) return;
    const uint32_t i = list[q];
    uint8_t *nd = nodes + (size_t)i * Lay::kStride;
    int32_t ref[N]; bool used[N]; RBox box[N], all;
    set_empty(all);
    for (int c = 0; c < N; ++c) {
        ref[c] = Lay::ref(nd, c);
        used[c] = ref[c] != kEmptyRef;
        if (!used[c]) { carea[(size_t)i * N + c] = 0.f; continue; }
        set_empty(box[c]);
        if (ref[c] >= 0) grow(box[c], nbox + (size_t)ref[c] * 6); // an inner child: its level ran before this one
        else {
            const uint32_t enc = (uint32_t)~ref[c], first = enc >> 3, cnt = (enc & 7u) + 1u;
            for (uint32_t j = 0; j < cnt; ++j) grow(box[c], tbox + (size_t)(first + j) * 6);
        }
        carea[(size_t)i * N + c] = area_of(box[c]);
        for (int k = 0; k < 3; ++k) { all.lo[k] = fminf(all.lo[k], box[c].lo[k]); all.hi[k] = fmaxf(all.hi[k], box[c].hi[k]); }
    }
    for (int k = 0; k < 3; ++k) { nbox[(size_t)i * 6 + k] = all.lo[k]; nbox[(size_t)i * 6 + 3 + k] = all.hi[k]; }
    if constexpr (Lay::Q) quantize_node<N>(box, used, reinterpret_cast<uint32_t *>(nd)); // refs and slot order stay (layout 73: octant slots)
    else {
        float4 *row = reinterpret_cast<float4 *>(nd);
        for (int c = 0; c < N; ++c) {
            if (!used[c]) continue;
            row[2 * c] = make_float4(box[c].lo[0], box[c].lo[1], box[c].lo[2], __int_as_float(ref[c]));
            row[2 * c + 1] = make_float4(box[c].hi[0], box[c].hi[1], box[c].hi[2], 0.f);
        }
    }
}

// bvh_build.cpp emit_blob: sum over child slots of area / root area (f32 quotient), times the triangle count for a leaf child, in double
template <int L>
__global__ void __launch_bounds__(kBlock) k_refit_sah(const uint8_t *__restrict__ nodes, uint32_t n_nodes, const float *__restrict__ carea,
                                                      const float *__restrict__ nbox, double *__restrict__ partial)
{
    using Lay = Layout<L>;
    __shared__ double red[kBlock];
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    double v = 0.0;
    if (i < n_nodes) {
        RBox root;
        for (int k = 0; k < 3; ++k) { root.lo[k] = nbox[k]; root.hi[k] = nbox[3 + k]; }
        const float ra = fmaxf(area_of(root), 1e-30f);
        const uint8_t *nd = nodes + (size_t)i * Lay::kStride;
        for (int c = 0; c < Lay::N; ++c) {
            const int32_t r = Lay::ref(nd, c);
            if (r == kEmptyRef) continue;
            v += (double)(carea[(size_t)i * Lay::N + c] / ra) * (double)(r < 0 ? ((uint32_t)~r & 7u) + 1u : 1u);
        }
    }
    red[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t s = kBlock / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

__global__ void __launch_bounds__(kBlock) k_refit_sum(const double *__restrict__ partial, uint32_t n, double *__restrict__ out)
{
    __shared__ double red[kBlock];
    double v = 0.0;
    for (uint32_t i = threadIdx.x; i < n; i += kBlock) v += partial[i];
    red[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t s = kBlock / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = red[0];
}

dim3 blocks_for(uint64_t n) { return dim3((uint32_t)((n + kBlock - 1) / kBlock)); }

} // namespace

bool refit_levels(const int32_t *refs, uint32_t n_nodes, uint32_t fan, uint32_t n_tris, std::vector<uint32_t> &list, std::vector<uint32_t> &off)
{
    list.clear(); off.assign(1, 0u);
    if (n_nodes == 0) return true;
    std::vector<std::vector<uint32_t>> levels(1, std::vector<uint32_t>{ 0u });
    std::vector<uint8_t> seen(n_nodes, 0);
    seen[0] = 1;
    size_t total = 1;
    while (!levels.back().empty()) {
        std::vector<uint32_t> next;
        for (const uint32_t i : levels.back())
            for (uint32_t c = 0; c < fan; ++c) {
                const int32_t r = refs[(size_t)i * fan + c];
                if (r == kEmptyRef) continue;
                if (r >= 0) {
                    if ((uint32_t)r >= n_nodes || seen[r]) return false;
                    seen[r] = 1;
                    next.push_back((uint32_t)r);
                } else {
                    const uint32_t enc = (uint32_t)~r;
                    if ((uint64_t)(enc >> 3) + (enc & 7u) + 1u > n_tris) return false;
                }
            }
        total += next.size();
        levels.push_back(std::move(next));
    }
    levels.pop_back();
    if (total != n_nodes) return false;
    list.reserve(n_nodes);
    for (size_t l = levels.size(); l-- > 0;) {
        list.insert(list.end(), levels[l].begin(), levels[l].end());
        off.push_back((uint32_t)list.size());
    }
    return true;
}

hipError_t launch_refit_stage(hipStream_t s, const float *in, float *out, uint64_t n_floats, uint32_t *bad)
{
    if (!n_floats) return hipSuccess;
    const uint64_t want = (n_floats + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_refit_stage, dim3((uint32_t)(want < 8192 ? want : 8192)), dim3(kBlock), 0, s, in, out, n_floats, bad);
    return hipGetLastError();
}

hipError_t launch_refit_tris(hipStream_t s, const float *verts9, float4 *rec, uint32_t n_tris, float *tbox)
{
    if (!n_tris) return hipSuccess;
    hipLaunchKernelGGL(k_refit_tris, blocks_for(n_tris), dim3(kBlock), 0, s, verts9, rec, n_tris, tbox);
    return hipGetLastError();
}

hipError_t launch_refit_level(hipStream_t s, uint32_t layout, void *nodes, const uint32_t *list, uint32_t count, const float *tbox,
                              float *nbox, float *carea)
{
    if (!count) return hipSuccess;
    uint8_t *nd = static_cast<uint8_t *>(nodes);
    switch (layout) {
    case PT_BVH_WIDTH_2:  hipLaunchKernelGGL(k_refit_level<PT_BVH_WIDTH_2>, blocks_for(count), dim3(kBlock), 0, s, nd, list, count, tbox, nbox, carea); break;
    case PT_BVH_WIDTH_4:  hipLaunchKernelGGL(k_refit_level<PT_BVH_WIDTH_4>, blocks_for(count), dim3(kBlock), 0, s, nd, list, count, tbox, nbox, carea); break;
    case PT_BVH_WIDTH_4Q: hipLaunchKernelGGL(k_refit_level<PT_BVH_WIDTH_4Q>, blocks_for(count), dim3(kBlock), 0, s, nd, list, count, tbox, nbox, carea); break;
    case PT_BVH_WIDTH_8Q:
    case PT_BVH_WIDTH_8O: hipLaunchKernelGGL(k_refit_level<PT_BVH_WIDTH_8Q>, blocks_for(count), dim3(kBlock), 0, s, nd, list, count, tbox, nbox, carea); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

uint32_t refit_sah_blocks(uint32_t n_nodes) { return n_nodes ? (n_nodes + kBlock - 1) / kBlock : 1u; }

hipError_t launch_refit_sah(hipStream_t s, uint32_t layout, const void *nodes, uint32_t n_nodes, const float *carea, const float *nbox,
                            double *partial, double *out)
{
    if (!n_nodes) return hipMemsetAsync(out, 0, sizeof(double), s);
    const uint8_t *nd = static_cast<const uint8_t *>(nodes);
    const dim3 g = blocks_for(n_nodes);
    switch (layout) {
    case PT_BVH_WIDTH_2:  hipLaunchKernelGGL(k_refit_sah<PT_BVH_WIDTH_2>, g, dim3(kBlock), 0, s, nd, n_nodes, carea, nbox, partial); break;
    case PT_BVH_WIDTH_4:  hipLaunchKernelGGL(k_refit_sah<PT_BVH_WIDTH_4>, g, dim3(kBlock), 0, s, nd, n_nodes, carea, nbox, partial); break;
    case PT_BVH_WIDTH_4Q: hipLaunchKernelGGL(k_refit_sah<PT_BVH_WIDTH_4Q>, g, dim3(kBlock), 0, s, nd, n_nodes, carea, nbox, partial); break;
    case PT_BVH_WIDTH_8Q:
    case PT_BVH_WIDTH_8O: hipLaunchKernelGGL(k_refit_sah<PT_BVH_WIDTH_8Q>, g, dim3(kBlock), 0, s, nd, n_nodes, carea, nbox, partial); break;
    default: return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(k_refit_sum, dim3(1), dim3(kBlock), 0, s, partial, g.x, out);
    return hipGetLastError();
}

} // namespace ptrt
