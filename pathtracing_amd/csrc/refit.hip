// refit.hip — pt_scene_update_triangles on the device (docs/SPEC.md §4.3). The committed tree keeps its topology, its leaf assignment
// and its memory order; only the numbers change:
//   k_refit_stage : device input -> the scene's spare vertex buffer, with a flag for any non-finite coordinate (read before anything of
//                   the scene is written)
//   k_refit_tris  : every triangle record rewritten from the new vertices, and its padded box
//   k_refit_level : one launch per tree level, deepest first: a node's child boxes from its leaves' triangle boxes and its inner children's
//                   unions, written as f32 slots or re-quantised
//   k_refit_sah   : the builder's SAH cost of the new boxes, reduced in a fixed order
// Every box is an exact union (min / max) of padded triangle boxes made from the input vertices, which is what every builder puts in
// the blob, so the refitted blob is a blob a builder could have emitted for the new vertices: it renders that commit's picture (§4.1).
// Record, box, quantiser, node layouts and SAH term are blob_rules.h's, the text the builders run.
#include <hip/hip_runtime.h>
#include <type_traits>
#include "refit.h"
#include "blob_rules.h"

namespace ptrt {
namespace {

constexpr uint32_t kBlock = 256;

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
    float r[16];
    tri_record(p, id, __float_as_uint(r1.w), r); // the record keeps its id, its material and its place
    for (int k = 0; k < 4; ++k) rec[(size_t)j * 4 + k] = make_float4(r[4 * k], r[4 * k + 1], r[4 * k + 2], r[4 * k + 3]);
    const Box b = tri_box(p); // the padded leaf box of docs/SPEC.md §4.1, from the input vertices
    for (int k = 0; k < 3; ++k) { tbox[(size_t)j * 6 + k] = b.lo[k]; tbox[(size_t)j * 6 + 3 + k] = b.hi[k]; }
}

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
    int32_t ref[N]; bool used[N]; Box box[N], all = Box::empty();
    for (int c = 0; c < N; ++c) {
        ref[c] = Lay::ref(nd, c);
        used[c] = ref[c] != kEmptyRef;
        if (!used[c]) { carea[(size_t)i * N + c] = 0.f; continue; }
        box[c] = Box::empty();
        if (ref[c] >= 0) box[c].grow(Box::of(nbox + (size_t)ref[c] * 6)); // an inner child: its level ran before this one
        else
            for (uint32_t j = 0; j < leaf_count(ref[c]); ++j) box[c].grow(Box::of(tbox + (size_t)(leaf_first(ref[c]) + j) * 6));
        carea[(size_t)i * N + c] = box[c].area();
        all.grow(box[c]);
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

// the builder's SAH cost: blob_rules.h sah_child_term over every child slot, summed in double
template <int L>
__global__ void __launch_bounds__(kBlock) k_refit_sah(const uint8_t *__restrict__ nodes, uint32_t n_nodes, const float *__restrict__ carea,
                                                      const float *__restrict__ nbox, double *__restrict__ partial)
{
    using Lay = Layout<L>;
    __shared__ double red[kBlock];
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    double v = 0.0;
    if (i < n_nodes) {
        const float ra = sah_root_area(Box::of(nbox));
        const uint8_t *nd = nodes + (size_t)i * Lay::kStride;
        for (int c = 0; c < Lay::N; ++c) {
            const int32_t r = Lay::ref(nd, c);
            if (r == kEmptyRef) continue;
            v += sah_child_term(carea[(size_t)i * Lay::N + c], ra, r);
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

// layout code -> template argument, for this file's kernels: f(constant) with the layout whose node format the code names (8O is the 8Q
// node with its children in octant slots). False: no such layout.
template <class F> bool with_node_layout(uint32_t layout, F f)
{
    switch (layout) {
    case PT_BVH_WIDTH_2:  f(std::integral_constant<int, PT_BVH_WIDTH_2>{}); return true;
    case PT_BVH_WIDTH_4:  f(std::integral_constant<int, PT_BVH_WIDTH_4>{}); return true;
    case PT_BVH_WIDTH_4Q: f(std::integral_constant<int, PT_BVH_WIDTH_4Q>{}); return true;
    case PT_BVH_WIDTH_8Q:
    case PT_BVH_WIDTH_8O: f(std::integral_constant<int, PT_BVH_WIDTH_8Q>{}); return true;
    default: return false;
    }
}

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
                    if ((uint64_t)leaf_first(r) + leaf_count(r) > n_tris) return false;
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
    if (!with_node_layout(layout, [&](auto L) { hipLaunchKernelGGL(k_refit_level<decltype(L)::value>, blocks_for(count), dim3(kBlock), 0, s, nd, list, count, tbox, nbox, carea); }))
        return hipErrorInvalidValue;
    return hipGetLastError();
}

uint32_t refit_sah_blocks(uint32_t n_nodes) { return n_nodes ? (n_nodes + kBlock - 1) / kBlock : 1u; }

hipError_t launch_refit_sah(hipStream_t s, uint32_t layout, const void *nodes, uint32_t n_nodes, const float *carea, const float *nbox,
                            double *partial, double *out)
{
    if (!n_nodes) return hipMemsetAsync(out, 0, sizeof(double), s);
    const uint8_t *nd = static_cast<const uint8_t *>(nodes);
    const dim3 g = blocks_for(n_nodes);
    if (!with_node_layout(layout, [&](auto L) { hipLaunchKernelGGL(k_refit_sah<decltype(L)::value>, g, dim3(kBlock), 0, s, nd, n_nodes, carea, nbox, partial); }))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_refit_sum, dim3(1), dim3(kBlock), 0, s, partial, g.x, out);
    return hipGetLastError();
}

} // namespace ptrt
