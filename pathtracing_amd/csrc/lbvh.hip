// lbvh.hip — GPU construction of a binary LBVH (the reference has no acceleration structure).
//   k_tri_boxes   : per triangle, the padded box of docs/SPEC.md §4.1 and its centroid; scene centroid bounds by atomics
//   k_morton      : 30-bit Morton code of the centroid
//   (rocPRIM)     : radix sort of (code, triangle) pairs
//   k_hierarchy   : Karras 2012 — one thread per internal node finds its key range and split by binary search on the
//                   common-prefix length (ties between equal codes are broken by the index, so duplicates form a balanced subtree)
//   k_refit       : leaves walk up; the second arrival at a node unites the children's boxes (agent-scope fences between)
// Then either build_lbvh_blob4q_device packs the default BVH4Q blob right here on the device (second half of this file), or — other
// node layouts — the binary tree is copied back and packed by build_bvh_from_binary() on the host. The closest hit does not depend
// on the tree (SPEC §4), so a scene committed with this builder renders the same picture bit for bit.
#include <cstring> // rocprim's texture_cache_iterator.hpp needs ::memset
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include <algorithm>
#include <chrono>
#include <vector>
#include "bvh_build.h"
#include "blob_rules.h"

namespace ptrt {
namespace {

__device__ __forceinline__ uint32_t f_ord(float f) { const uint32_t b = __float_as_uint(f); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
inline float f_unord(uint32_t u) { const uint32_t b = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u; float f; std::memcpy(&f, &b, 4); return f; }

__global__ void __launch_bounds__(256) k_tri_boxes(const float *__restrict__ verts, uint32_t n, float *__restrict__ leaf_box,
                                                   float *__restrict__ cent, uint32_t *__restrict__ bounds /* 3 min, 3 max (ordered uints) */)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float c[3];
    const Box b = tri_box(verts + (size_t)i * 9, c);
    for (int k = 0; k < 3; ++k) {
        leaf_box[(size_t)i * 6 + k] = b.lo[k];
        leaf_box[(size_t)i * 6 + 3 + k] = b.hi[k];
        cent[(size_t)i * 3 + k] = c[k];
        atomicMin(&bounds[k], f_ord(c[k]));
        atomicMax(&bounds[3 + k], f_ord(c[k]));
    }
}

__device__ __forceinline__ uint32_t spread10(uint32_t v)
{
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}

__global__ void __launch_bounds__(256) k_morton(const float *__restrict__ cent, uint32_t n, float3 cmin, float3 inv_ext,
                                                uint32_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float x = (cent[(size_t)i * 3 + 0] - cmin.x) * inv_ext.x, y = (cent[(size_t)i * 3 + 1] - cmin.y) * inv_ext.y,
                z = (cent[(size_t)i * 3 + 2] - cmin.z) * inv_ext.z;
    const uint32_t xi = (uint32_t)fminf(fmaxf(x * 1024.0f, 0.0f), 1023.0f), yi = (uint32_t)fminf(fmaxf(y * 1024.0f, 0.0f), 1023.0f),
                   zi = (uint32_t)fminf(fmaxf(z * 1024.0f, 0.0f), 1023.0f);
    keys[i] = (spread10(xi) << 2) | (spread10(yi) << 1) | spread10(zi);
    vals[i] = i;
}

__device__ __forceinline__ int delta(const uint32_t *__restrict__ keys, int n, int i, int j)
{
    if (j < 0 || j >= n) return -1;
    const uint32_t a = keys[i], b = keys[j];
    return a == b ? 32 + __clz((uint32_t)(i ^ j)) : __clz(a ^ b);
}

// children: >= 0 internal node, < 0 leaf ~j (j = position in the sorted order)
__global__ void __launch_bounds__(256) k_hierarchy(const uint32_t *__restrict__ keys, int n, int32_t *__restrict__ left, int32_t *__restrict__ right,
                                                   uint32_t *__restrict__ first, uint32_t *__restrict__ last,
                                                   int32_t *__restrict__ parent_node, int32_t *__restrict__ parent_leaf)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n - 1) return;
    const int d = (delta(keys, n, i, i + 1) - delta(keys, n, i, i - 1)) >= 0 ? 1 : -1;
    const int dmin = delta(keys, n, i, i - d);
    int lmax = 2;
    while (delta(keys, n, i, i + lmax * d) > dmin) lmax <<= 1;
    int l = 0;
    for (int t = lmax >> 1; t >= 1; t >>= 1)
        if (delta(keys, n, i, i + (l + t) * d) > dmin) l += t;
    const int j = i + l * d;
    const int dnode = delta(keys, n, i, j);
    int s = 0, t = l;
    do {
        t = (t + 1) >> 1;
        if (delta(keys, n, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    const int gamma = i + s * d + (d < 0 ? d : 0);
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    const int32_t lc = (lo == gamma) ? ~gamma : gamma, rc = (hi == gamma + 1) ? ~(gamma + 1) : gamma + 1;
    left[i] = lc; right[i] = rc; first[i] = (uint32_t)lo; last[i] = (uint32_t)hi;
    if (lc >= 0) parent_node[lc] = i; else parent_leaf[~lc] = i;
    if (rc >= 0) parent_node[rc] = i; else parent_leaf[~rc] = i;
    if (i == 0) parent_node[0] = -1;
}

__global__ void __launch_bounds__(256) k_refit(const uint32_t *__restrict__ order, const float *__restrict__ leaf_box, int n,
                                               const int32_t *__restrict__ left, const int32_t *__restrict__ right,
                                               const int32_t *__restrict__ parent_node, const int32_t *__restrict__ parent_leaf,
                                               float *__restrict__ node_box, uint32_t *__restrict__ arrived)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    int cur = parent_leaf[j];
    while (cur >= 0) {
        __threadfence();                                 // release what this thread (or its child visit) wrote
        if (atomicAdd(&arrived[cur], 1u) == 0u) return;  // first of the two children to arrive: the sibling finishes the node
        __threadfence();                                 // acquire the sibling subtree's boxes
        float b[6];
        const int32_t c[2] = { left[cur], right[cur] };
        for (int k = 0; k < 3; ++k) { b[k] = __builtin_inff(); b[3 + k] = -__builtin_inff(); }
        for (int s = 0; s < 2; ++s) {
            const float *src = c[s] >= 0 ? node_box + (size_t)c[s] * 6 : leaf_box + (size_t)order[~c[s]] * 6;
            for (int k = 0; k < 3; ++k) {
                b[k] = fminf(b[k], __hip_atomic_load(src + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                b[3 + k] = fmaxf(b[3 + k], __hip_atomic_load(src + 3 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            }
        }
        for (int k = 0; k < 6; ++k) __hip_atomic_store(node_box + (size_t)cur * 6 + k, b[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        cur = parent_node[cur];
    }
}

#define LB_TRY(x) do { hipError_t _e = (x); if (_e != hipSuccess) return _e; } while (0)

// The binary LBVH on the device: construction shared by the two consumers below.
struct Lbvh {
    uint32_t n = 0;
    DevBuf<float> verts, leaf_box, cent, node_box;
    DevBuf<uint32_t> bounds, keys, vals, keys2, order, first, last, arrived;
    DevBuf<int32_t> left, right, pn, pl;
    DevBuf<unsigned char> tmp;
    hipError_t construct(hipStream_t stream, const float *verts9, uint32_t n_)
    {
        n = n_;
        LB_TRY(verts.ensure((size_t)n * 9)); LB_TRY(leaf_box.ensure((size_t)n * 6)); LB_TRY(cent.ensure((size_t)n * 3));
        LB_TRY(node_box.ensure((size_t)(n - 1) * 6)); LB_TRY(bounds.ensure(6));
        LB_TRY(keys.ensure(n)); LB_TRY(vals.ensure(n)); LB_TRY(keys2.ensure(n)); LB_TRY(order.ensure(n));
        LB_TRY(first.ensure(n - 1)); LB_TRY(last.ensure(n - 1)); LB_TRY(arrived.ensure(n - 1));
        LB_TRY(left.ensure(n - 1)); LB_TRY(right.ensure(n - 1)); LB_TRY(pn.ensure(n - 1)); LB_TRY(pl.ensure(n));
        LB_TRY(hipMemcpyAsync(verts.p, verts9, (size_t)n * 36, hipMemcpyHostToDevice, stream));
        const uint32_t init_bounds[6] = { 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u };
        LB_TRY(hipMemcpyAsync(bounds.p, init_bounds, sizeof init_bounds, hipMemcpyHostToDevice, stream));
        LB_TRY(hipMemsetAsync(arrived.p, 0, (size_t)(n - 1) * 4, stream));
        const dim3 grid((n + 255) / 256), block(256);
        hipLaunchKernelGGL(k_tri_boxes, grid, block, 0, stream, verts.p, n, leaf_box.p, cent.p, bounds.p);
        uint32_t hb[6];
        LB_TRY(hipMemcpyAsync(hb, bounds.p, sizeof hb, hipMemcpyDeviceToHost, stream));
        LB_TRY(hipStreamSynchronize(stream));
        const float lo[3] = { f_unord(hb[0]), f_unord(hb[1]), f_unord(hb[2]) }, hi[3] = { f_unord(hb[3]), f_unord(hb[4]), f_unord(hb[5]) };
        const float3 cmin = make_float3(lo[0], lo[1], lo[2]);
        const float3 inv = make_float3(hi[0] > lo[0] ? 1.0f / (hi[0] - lo[0]) : 0.f, hi[1] > lo[1] ? 1.0f / (hi[1] - lo[1]) : 0.f, hi[2] > lo[2] ? 1.0f / (hi[2] - lo[2]) : 0.f);
        hipLaunchKernelGGL(k_morton, grid, block, 0, stream, cent.p, n, cmin, inv, keys.p, vals.p);
        size_t tmp_bytes = 0;
        LB_TRY(rocprim::radix_sort_pairs(nullptr, tmp_bytes, keys.p, keys2.p, vals.p, order.p, (size_t)n, 0, 30, stream));
        LB_TRY(tmp.ensure(tmp_bytes));
        LB_TRY(rocprim::radix_sort_pairs(tmp.p, tmp_bytes, keys.p, keys2.p, vals.p, order.p, (size_t)n, 0, 30, stream));
        hipLaunchKernelGGL(k_hierarchy, dim3((n - 1 + 255) / 256), block, 0, stream, keys2.p, (int)n, left.p, right.p, first.p, last.p, pn.p, pl.p);
        hipLaunchKernelGGL(k_refit, grid, block, 0, stream, order.p, leaf_box.p, (int)n, left.p, right.p, pn.p, pl.p, node_box.p, arrived.p);
        return hipGetLastError();
    }
};

// =================================================================================================
// Packing on the device: binary LBVH -> BVH4Q blob (64-byte quantised nodes, breadth-first) + 64-byte triangle records, without
// the tree ever visiting the host. Only the top storey does: the LBVH is cut into clusters of <= kClusterTris triangles, their
// boxes (a few thousand) go to the host's binned-SAH builder and the small binary tree over them comes back (bvh_build.cpp has the
// same two-storey scheme for the other node layouts). Then, level by level: expand every node of the level to <= 4 children by
// opening the child of largest area, scan the inner children to number the next level breadth-first, quantise and write the node.
// (Opening by area is a deliberate difference from the host: emit_blob chooses a wide node's children by the SAH-optimal dynamic
// programme, which needs the costs of whole subtrees; the device keeps the local rule. DESIGN.md §7.) Triangles are emitted in Morton
// order, so every leaf's range [first, last] is contiguous as it is. The leaf rule and the depth / stack-need rule are blob_rules.h's.
using Lay = Layout<PT_BVH_WIDTH_4Q>;     // the one layout packed here
constexpr int32_t kTopBase = 0x40000000;  // binary refs: >= kTopBase top-storey node, 0 .. n-2 LBVH node, < 0 LBVH leaf ~j

struct TreeView {
    const int32_t *left, *right; const uint32_t *first, *last, *order; const float *node_box, *leaf_box; const uint8_t *leaf_flag;
    const int32_t *top_left, *top_right; const float *top_box;
};
__device__ __forceinline__ Box box_of(const TreeView &t, int32_t r)
{
    return Box::of(r >= kTopBase ? t.top_box + (size_t)(r - kTopBase) * 6 : r >= 0 ? t.node_box + (size_t)r * 6 : t.leaf_box + (size_t)t.order[~r] * 6);
}
__device__ __forceinline__ uint32_t count_of(const TreeView &t, int32_t r) { return r < 0 ? 1u : t.last[r] - t.first[r] + 1u; } // LBVH refs only
__device__ __forceinline__ bool blob_leaf(const TreeView &t, int32_t r) { return r < 0 || (r < kTopBase && t.leaf_flag[r]); }

// per LBVH node: does it become a leaf of the blob (blob_rules.h lbvh_leaf)? and is it a cluster root?
__global__ void __launch_bounds__(256) k_mark(TreeView t, uint32_t n, uint32_t cluster_tris, const int32_t *__restrict__ parent_node,
                                              const int32_t *__restrict__ parent_leaf, uint8_t *__restrict__ leaf_flag, int32_t *__restrict__ clusters,
                                              uint32_t *__restrict__ n_clusters)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n - 1) {
        const uint32_t cnt = t.last[i] - t.first[i] + 1u;
        bool leaf = false;
        if (cnt <= kMaxLeaf) { // (the rule says so itself: asked here first, a bigger node's boxes stay unread)
            const int32_t l = t.left[i], r = t.right[i];
            leaf = lbvh_leaf(cnt, box_of(t, (int32_t)i).area(), count_of(t, l), box_of(t, l).area(), count_of(t, r), box_of(t, r).area());
        }
        leaf_flag[i] = leaf ? 1 : 0;
        const int32_t p = parent_node[i];
        if (cnt <= cluster_tris && (p < 0 || t.last[p] - t.first[p] + 1u > cluster_tris)) clusters[atomicAdd(n_clusters, 1u)] = (int32_t)i;
    }
    if (i < n) { // single triangles hanging off a node that is too big to be a cluster
        const int32_t p = parent_leaf[i];
        if (t.last[p] - t.first[p] + 1u > cluster_tris) clusters[atomicAdd(n_clusters, 1u)] = ~(int32_t)i;
    }
}

__global__ void __launch_bounds__(256) k_cluster_info(TreeView t, const int32_t *__restrict__ clusters, uint32_t nc, float *__restrict__ boxes, uint32_t *__restrict__ firsts)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nc) return;
    const int32_t r = clusters[i];
    const Box b = box_of(t, r);
    for (int k = 0; k < 3; ++k) { boxes[(size_t)i * 6 + k] = b.lo[k]; boxes[(size_t)i * 6 + 3 + k] = b.hi[k]; }
    firsts[i] = r < 0 ? (uint32_t)~r : t.first[r];
}

// one level, first half: the (up to) 4 children of every node of the level, and how many of them are inner nodes
__global__ void __launch_bounds__(256) k_expand(TreeView t, const int32_t *__restrict__ queue, uint32_t n_cur, uint32_t base, int32_t *__restrict__ kids,
                                                uint32_t *__restrict__ inner_count)
{
    const uint32_t q = blockIdx.x * 256 + threadIdx.x;
    if (q >= n_cur) return;
    const int32_t r = queue[q];
    int32_t kid[4] = { kEmptyRef, kEmptyRef, kEmptyRef, kEmptyRef };
    int nk = 0;
    if (blob_leaf(t, r)) kid[nk++] = r; // (the whole scene is one leaf) single child
    else {
        kid[0] = r >= kTopBase ? t.top_left[r - kTopBase] : t.left[r];
        kid[1] = r >= kTopBase ? t.top_right[r - kTopBase] : t.right[r];
        nk = 2;
        while (nk < 4) {
            int best = -1; float ba = -1.f;
            for (int i = 0; i < nk; ++i)
                if (!blob_leaf(t, kid[i])) { const float a = box_of(t, kid[i]).area(); if (a > ba) { ba = a; best = i; } }
            if (best < 0) break;
            const int32_t c = kid[best];
            for (int i = nk; i > best + 1; --i) kid[i] = kid[i - 1];
            kid[best] = c >= kTopBase ? t.top_left[c - kTopBase] : t.left[c];
            kid[best + 1] = c >= kTopBase ? t.top_right[c - kTopBase] : t.right[c];
            nk++;
        }
    }
    uint32_t ni = 0;
    for (int i = 0; i < 4; ++i) {
        kids[(size_t)(base + q) * 4 + i] = kid[i];
        if (kid[i] != kEmptyRef && !blob_leaf(t, kid[i])) ++ni;
    }
    inner_count[q] = ni;
}

// one level, second half: number the inner children breadth-first (they are the next level's queue), quantise, write the node
__global__ void __launch_bounds__(256) k_finalize(TreeView t, uint32_t n_cur, uint32_t base, const int32_t *__restrict__ kids, const uint32_t *__restrict__ offs,
                                                  int32_t *__restrict__ queue_next, uint8_t *__restrict__ nodes, float *__restrict__ cost, float inv_root_area)
{
    const uint32_t q = blockIdx.x * 256 + threadIdx.x;
    if (q >= n_cur) return;
    const uint32_t node = base + q;
    int32_t ref[4];
    Box box[4];
    uint32_t rank = 0;
    float my_cost = 0.f;
    for (int c = 0; c < 4; ++c) {
        const int32_t k = kids[(size_t)node * 4 + c];
        if (k == kEmptyRef) { ref[c] = kEmptyRef; continue; }
        box[c] = box_of(t, k);
        if (blob_leaf(t, k)) {
            const uint32_t first = k < 0 ? (uint32_t)~k : t.first[k], cnt = count_of(t, k);
            ref[c] = leaf_ref(first, cnt);
            my_cost += box[c].area() * inv_root_area * (float)cnt;
        } else {
            const uint32_t pos = offs[q] + rank++;
            queue_next[pos] = k;
            ref[c] = (int32_t)(base + n_cur + pos);
            my_cost += box[c].area() * inv_root_area;
        }
    }
    cost[node] = my_cost;
    // ---- docs/SPEC.md §4.1 BVH4Q: quantise the children's boxes (blob_rules.h, shared with the host builder and refit.hip), then the refs
    bool used[4];
    for (int c = 0; c < 4; ++c) used[c] = ref[c] != kEmptyRef;
    uint32_t *w = reinterpret_cast<uint32_t *>(nodes + (size_t)node * Lay::kStride);
    quantize_node<4>(box, used, w);
    for (int c = 0; c < 4; ++c) w[4 + c] = (uint32_t)ref[c];
}

// depth and worst-case traversal-stack need, one level at a time from the bottom (children live in the next level)
__global__ void __launch_bounds__(256) k_depth(const uint8_t *__restrict__ nodes, uint32_t base, uint32_t n_cur, uint32_t *__restrict__ depth, uint32_t *__restrict__ need)
{
    const uint32_t q = blockIdx.x * 256 + threadIdx.x;
    if (q >= n_cur) return;
    DepthNeed f;
    for (int c = 0; c < Lay::N; ++c) f.child(Lay::ref(nodes + (size_t)(base + q) * Lay::kStride, c), depth, need);
    depth[base + q] = f.depth();
    need[base + q] = f.need();
}

// the device triangle record (one 64-byte line, Morton order): blob_rules.h tri_record, as scene.cpp makes it for the host-built trees
__global__ void __launch_bounds__(256) k_tri_records(const float *__restrict__ verts, const uint32_t *__restrict__ mats, const uint32_t *__restrict__ order, uint32_t n,
                                                     float4 *__restrict__ rec)
{
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const uint32_t id = order[j];
    float r[16];
    tri_record(verts + (size_t)id * 9, id, mats ? mats[id] : 0u, r);
    for (int k = 0; k < 4; ++k) rec[(size_t)j * 4 + k] = make_float4(r[4 * k], r[4 * k + 1], r[4 * k + 2], r[4 * k + 3]);
}

// The device packer: the buffers of build_lbvh_blob4q_device and its four phases, in the order they run. A phase allocates what it is
// the first to need; the host waits for the stream twice in the cut, once per level and once at the end.
struct Packer {
    hipStream_t stream = nullptr;
    uint32_t n = 0;
    Lbvh t;
    TreeView tv{};
    static dim3 blocks(uint32_t k) { return dim3((k + 255) / 256); }
    // mark + cut
    DevBuf<uint8_t> leaf_flag; DevBuf<int32_t> clusters; DevBuf<uint32_t> n_clusters, mats, cfirst; DevBuf<float> cbox; DevBuf<float4> tris;
    uint32_t nc = 0;
    std::vector<int32_t> h_clusters; std::vector<float> h_cbox; std::vector<uint32_t> h_cfirst;
    // top storey
    DevBuf<int32_t> top_left, top_right; DevBuf<float> top_box;
    int32_t root_ref = 0; float root_area = 0.f;
    // levels
    DevBuf<uint8_t> nodes; DevBuf<int32_t> kids, queue_a, queue_b; DevBuf<uint32_t> inner_count, offs, depth, need; DevBuf<float> cost; DevBuf<unsigned char> scan_tmp;
    std::vector<uint32_t> level_base; // first node of every level, then n_nodes
    uint32_t n_nodes = 0;
    // figures
    DevBuf<float> sum; DevBuf<unsigned char> red_tmp; DevBuf<float4> final_nodes;

    // leaf flags and cluster roots; the clusters' roots, boxes and first triangles come to the host, the triangle records are started
    hipError_t mark_and_cut(const uint32_t *h_mats)
    {
        const dim3 block(256);
        LB_TRY(leaf_flag.ensure(n)); LB_TRY(clusters.ensure(n)); LB_TRY(n_clusters.ensure(1));
        LB_TRY(hipMemsetAsync(n_clusters.p, 0, 4, stream));
        if (h_mats) { LB_TRY(mats.ensure(n)); LB_TRY(hipMemcpyAsync(mats.p, h_mats, (size_t)n * 4, hipMemcpyHostToDevice, stream)); }
        tv = TreeView{ t.left.p, t.right.p, t.first.p, t.last.p, t.order.p, t.node_box.p, t.leaf_box.p, leaf_flag.p, nullptr, nullptr, nullptr };
        hipLaunchKernelGGL(k_mark, blocks(n), block, 0, stream, tv, n, kClusterTris, t.pn.p, t.pl.p, leaf_flag.p, clusters.p, n_clusters.p);
        LB_TRY(hipMemcpyAsync(&nc, n_clusters.p, 4, hipMemcpyDeviceToHost, stream));
        LB_TRY(hipStreamSynchronize(stream));
        if (nc == 0 || nc > n) return hipErrorUnknown;
        LB_TRY(cbox.ensure((size_t)nc * 6)); LB_TRY(cfirst.ensure(nc));
        hipLaunchKernelGGL(k_cluster_info, blocks(nc), block, 0, stream, tv, clusters.p, nc, cbox.p, cfirst.p);
        h_clusters.resize(nc); h_cbox.resize((size_t)nc * 6); h_cfirst.resize(nc);
        LB_TRY(hipMemcpyAsync(h_clusters.data(), clusters.p, (size_t)nc * 4, hipMemcpyDeviceToHost, stream));
        LB_TRY(hipMemcpyAsync(h_cbox.data(), cbox.p, (size_t)nc * 24, hipMemcpyDeviceToHost, stream));
        LB_TRY(hipMemcpyAsync(h_cfirst.data(), cfirst.p, (size_t)nc * 4, hipMemcpyDeviceToHost, stream));
        // the triangle records need nothing of the above: they run while the host builds the top storey
        LB_TRY(tris.ensure((size_t)n * 4));
        hipLaunchKernelGGL(k_tri_records, blocks(n), block, 0, stream, t.verts.p, h_mats ? mats.p : nullptr, t.order.p, n, tris.p);
        return hipStreamSynchronize(stream);
    }

    // on the host: binned SAH over the cluster boxes, in Morton order of the clusters (k_mark's append order is not deterministic)
    hipError_t top_storey()
    {
        std::vector<uint32_t> perm(nc);
        for (uint32_t i = 0; i < nc; ++i) perm[i] = i;
        std::sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return h_cfirst[a] < h_cfirst[b]; });
        std::vector<float> sorted_box((size_t)nc * 6);
        for (uint32_t i = 0; i < nc; ++i) std::memcpy(&sorted_box[(size_t)i * 6], &h_cbox[(size_t)perm[i] * 6], 24);
        std::vector<int32_t> left, right; std::vector<float> box; int32_t root = 0;
        build_sah_over_boxes(sorted_box.data(), nc, left, right, box, root);
        auto to_ref = [&](int32_t c) { return c < 0 ? h_clusters[perm[(uint32_t)~c]] : kTopBase + c; }; // SAH leaf ~i = cluster i
        for (auto &c : left) c = to_ref(c);
        for (auto &c : right) c = to_ref(c);
        root_ref = to_ref(root);
        root_area = sah_root_area(Box::of(root < 0 ? &sorted_box[(size_t)(uint32_t)~root * 6] : &box[(size_t)root * 6]));
        const size_t nt = left.size();
        LB_TRY(top_left.ensure(nt)); LB_TRY(top_right.ensure(nt)); LB_TRY(top_box.ensure(nt * 6));
        if (nt) {
            LB_TRY(hipMemcpyAsync(top_left.p, left.data(), nt * 4, hipMemcpyHostToDevice, stream));
            LB_TRY(hipMemcpyAsync(top_right.p, right.data(), nt * 4, hipMemcpyHostToDevice, stream));
            LB_TRY(hipMemcpyAsync(top_box.p, box.data(), nt * 24, hipMemcpyHostToDevice, stream));
        }
        tv.top_left = top_left.p; tv.top_right = top_right.p; tv.top_box = top_box.p;
        return hipSuccess;
    }

    // level by level: expand, scan, finalize. A 4-wide inner node has >= 2 children, so there are < n nodes in all.
    hipError_t pack_levels()
    {
        const dim3 block(256);
        const uint32_t cap = n;
        LB_TRY(nodes.ensure((size_t)cap * 64)); LB_TRY(kids.ensure((size_t)cap * 4)); LB_TRY(queue_a.ensure(cap)); LB_TRY(queue_b.ensure(cap));
        LB_TRY(inner_count.ensure(cap + 1)); LB_TRY(offs.ensure(cap + 1)); LB_TRY(depth.ensure(cap)); LB_TRY(need.ensure(cap)); LB_TRY(cost.ensure(cap));
        size_t scan_bytes = 0;
        LB_TRY(rocprim::exclusive_scan(nullptr, scan_bytes, inner_count.p, offs.p, 0u, (size_t)cap + 1, rocprim::plus<uint32_t>(), stream));
        LB_TRY(scan_tmp.ensure(scan_bytes));
        LB_TRY(hipMemcpyAsync(queue_a.p, &root_ref, 4, hipMemcpyHostToDevice, stream));
        uint32_t base = 0, n_cur = 1;
        int32_t *qc = queue_a.p, *qn = queue_b.p;
        while (n_cur) {
            if (base + n_cur > cap || level_base.size() > 200) return hipErrorUnknown;
            level_base.push_back(base);
            hipLaunchKernelGGL(k_expand, blocks(n_cur), block, 0, stream, tv, qc, n_cur, base, kids.p, inner_count.p);
            LB_TRY(hipMemsetAsync(inner_count.p + n_cur, 0, 4, stream)); // the scan's extra element: offs[n_cur] = the next level's size
            LB_TRY(rocprim::exclusive_scan(scan_tmp.p, scan_bytes, inner_count.p, offs.p, 0u, (size_t)n_cur + 1, rocprim::plus<uint32_t>(), stream));
            hipLaunchKernelGGL(k_finalize, blocks(n_cur), block, 0, stream, tv, n_cur, base, kids.p, offs.p, qn, nodes.p, cost.p, 1.0f / root_area);
            uint32_t n_next = 0;
            LB_TRY(hipMemcpyAsync(&n_next, offs.p + n_cur, 4, hipMemcpyDeviceToHost, stream));
            LB_TRY(hipStreamSynchronize(stream));
            base += n_cur; n_cur = n_next;
            std::swap(qc, qn);
        }
        n_nodes = base;
        level_base.push_back(n_nodes);
        return hipSuccess;
    }

    // depth and stack need from the deepest level up, the sum of the nodes' costs, and a node array of the exact size for the scene
    // (the work array is sized for the worst case)
    hipError_t figures(DeviceBlob4Q &out)
    {
        for (size_t l = level_base.size() - 1; l-- > 0;)
            hipLaunchKernelGGL(k_depth, blocks(level_base[l + 1] - level_base[l]), dim3(256), 0, stream, nodes.p, level_base[l], level_base[l + 1] - level_base[l], depth.p, need.p);
        size_t red_bytes = 0;
        LB_TRY(sum.ensure(1));
        LB_TRY(rocprim::reduce(nullptr, red_bytes, cost.p, sum.p, 0.f, (size_t)n_nodes, rocprim::plus<float>(), stream));
        LB_TRY(red_tmp.ensure(red_bytes));
        LB_TRY(rocprim::reduce(red_tmp.p, red_bytes, cost.p, sum.p, 0.f, (size_t)n_nodes, rocprim::plus<float>(), stream));
        LB_TRY(hipMemcpyAsync(&out.max_depth, depth.p, 4, hipMemcpyDeviceToHost, stream));
        LB_TRY(hipMemcpyAsync(&out.stack_need, need.p, 4, hipMemcpyDeviceToHost, stream));
        LB_TRY(hipMemcpyAsync(&out.sah_cost, sum.p, 4, hipMemcpyDeviceToHost, stream));
        LB_TRY(final_nodes.ensure((size_t)n_nodes * 4));
        LB_TRY(hipMemcpyAsync(final_nodes.p, nodes.p, (size_t)n_nodes * 64, hipMemcpyDeviceToDevice, stream));
        LB_TRY(hipStreamSynchronize(stream));
        LB_TRY(hipGetLastError());
        out.nodes = std::move(final_nodes); out.tris = std::move(tris);
        out.n_nodes = n_nodes;
        return hipSuccess;
    }
};

} // namespace

hipError_t build_lbvh_device(hipStream_t stream, const float *verts9, uint32_t n, BinaryBvh &out)
{
    const auto t0 = std::chrono::steady_clock::now();
    out = BinaryBvh{};
    if (n < 2) return hipErrorInvalidValue;
    Lbvh t;
    LB_TRY(t.construct(stream, verts9, n));
    auto fetch = [&](auto &v, const auto *src, size_t count) { v.resize(count); return hipMemcpyAsync(v.data(), src, count * sizeof *src, hipMemcpyDeviceToHost, stream); };
    LB_TRY(fetch(out.order, t.order.p, n));
    LB_TRY(fetch(out.left, t.left.p, n - 1)); LB_TRY(fetch(out.right, t.right.p, n - 1));
    LB_TRY(fetch(out.first, t.first.p, n - 1)); LB_TRY(fetch(out.last, t.last.p, n - 1));
    LB_TRY(fetch(out.box, t.node_box.p, (size_t)(n - 1) * 6));
    LB_TRY(hipStreamSynchronize(stream));
    out.device_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return hipSuccess;
}

hipError_t build_lbvh_blob4q_device(hipStream_t stream, const float *verts9, const uint32_t *mats, uint32_t n, DeviceBlob4Q &out)
{
    const auto t0 = std::chrono::steady_clock::now();
    out = DeviceBlob4Q{};
    if (n < 2) return hipErrorInvalidValue;
    Packer p;
    p.stream = stream; p.n = n;
    LB_TRY(p.t.construct(stream, verts9, n));
    LB_TRY(p.mark_and_cut(mats));
    LB_TRY(p.top_storey());
    LB_TRY(p.pack_levels());
    LB_TRY(p.figures(out));
    out.device_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return hipSuccess;
}

} // namespace ptrt
