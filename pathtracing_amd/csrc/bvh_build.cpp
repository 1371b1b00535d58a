// bvh_build.cpp — binned-SAH BVH2 build (16 bins/axis), optional SAH-area collapse to BVH4, breadth-first
// node layout (top levels contiguous => stageable in LDS, one 128-B line per BVH4 node). docs/SPEC.md §4.1. The blob's own rules — box,
// padding, leaf refs, triangle rows, quantiser, SAH term — are blob_rules.h's, shared with lbvh.hip and refit.hip.
#include "bvh_build.h"
#include "blob_rules.h"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <thread>

namespace ptrt {
namespace {

// Bins of the SAH sweep. Measured on the 1M-triangle Cornell (1080p / 64 spp): 16 / 32 / 64 bins = 7.72 / 7.63 / 7.60 node visits per
// ray, 17.60 / 17.48 / 17.37 ms per frame, 0.46 / 0.52 / 0.58 s per commit (the soup: 29.05 / 28.95 / 28.91 visits, 1.12 / 1.25 / 1.48 s).
#ifndef PT_SAH_BINS
#define PT_SAH_BINS 64
#endif
constexpr int kBins = PT_SAH_BINS;
constexpr float kInf = std::numeric_limits<float>::infinity();

struct Prim { Box box; float c[3]; };
struct Tmp { Box box; int32_t left, right; uint32_t first, count; }; // count > 0: leaf over idx[first, first+count)
inline void grow_point(Box &b, const float p[3]) { for (int k = 0; k < 3; ++k) { b.lo[k] = std::min(b.lo[k], p[k]); b.hi[k] = std::max(b.hi[k], p[k]); } }

struct Builder {
    const std::vector<Prim> &prims;
    std::vector<uint32_t> &idx;
    std::vector<Tmp> nodes;
    uint32_t max_leaf = kMaxLeaf; // 1: every primitive its own leaf (the top-level build over LBVH clusters)
    // Parallel build: ranges of more than `defer_above` primitives that reach depth `defer_depth` are not built but recorded in
    // `deferred` (a placeholder node holds their place); build_parallel() builds them on their own threads and splices them in.
    int defer_depth = -1; uint32_t defer_above = 0;
    struct Deferred { int32_t node; uint32_t b, e; int depth; };
    std::vector<Deferred> deferred;
    Builder(const std::vector<Prim> &p, std::vector<uint32_t> &i, size_t reserve) : prims(p), idx(i) { nodes.reserve(reserve); }
    Builder(const std::vector<Prim> &p, std::vector<uint32_t> &i) : Builder(p, i, p.size()) {}

    int32_t make_leaf(uint32_t b, uint32_t e, const Box &box)
    {
        Tmp t; t.box = box; t.left = t.right = -1; t.first = b; t.count = e - b;
        nodes.push_back(t);
        return (int32_t)nodes.size() - 1;
    }

    int32_t build(uint32_t b, uint32_t e, int depth)
    {
        const uint32_t n = e - b;
        if (depth == defer_depth && n > defer_above) {
            nodes.push_back(Tmp{});
            deferred.push_back(Deferred{ (int32_t)nodes.size() - 1, b, e, depth });
            return (int32_t)nodes.size() - 1;
        }
        Box box = Box::empty(), cb = Box::empty();
        for (uint32_t i = b; i < e; ++i) { box.grow(prims[idx[i]].box); grow_point(cb, prims[idx[i]].c); }
        if (n == 1) return make_leaf(b, e, box);

        uint32_t mid = 0;
        bool have_split = false;
        if (depth < 40) {
            float best = kInf; int best_axis = -1, best_bin = -1;
            for (int ax = 0; ax < 3; ++ax) {
                const float ext = cb.hi[ax] - cb.lo[ax];
                if (!(ext > 0.f)) continue;
                Box bb[kBins]; uint32_t cnt[kBins];
                for (int k = 0; k < kBins; ++k) { bb[k] = Box::empty(); cnt[k] = 0; }
                const float sc = (float)kBins / ext;
                for (uint32_t i = b; i < e; ++i) {
                    const Prim &p = prims[idx[i]];
                    int k = (int)((p.c[ax] - cb.lo[ax]) * sc);
                    k = std::min(std::max(k, 0), kBins - 1);
                    bb[k].grow(p.box); cnt[k]++;
                }
                float ra[kBins]; uint32_t rc[kBins];
                Box acc = Box::empty(); uint32_t c = 0;
                for (int k = kBins - 1; k >= 1; --k) { acc.grow(bb[k]); c += cnt[k]; ra[k] = acc.area(); rc[k] = c; }
                acc = Box::empty(); c = 0;
                for (int k = 0; k < kBins - 1; ++k) {
                    acc.grow(bb[k]); c += cnt[k];
                    if (c == 0 || rc[k + 1] == 0) continue;
                    const float cost = acc.area() * (float)c + ra[k + 1] * (float)rc[k + 1];
                    if (cost < best) { best = cost; best_axis = ax; best_bin = k; }
                }
            }
            const float leaf_cost = box.area() * (float)n;
            if (best_axis >= 0 && !(n <= max_leaf && best >= leaf_cost)) {
                const float ext = cb.hi[best_axis] - cb.lo[best_axis], sc = (float)kBins / ext, lo = cb.lo[best_axis];
                const int ax = best_axis, bin = best_bin;
                auto it = std::partition(idx.begin() + b, idx.begin() + e, [&](uint32_t id) {
                    int k = (int)((prims[id].c[ax] - lo) * sc);
                    k = std::min(std::max(k, 0), kBins - 1);
                    return k <= bin;
                });
                mid = (uint32_t)(it - idx.begin());
                have_split = mid > b && mid < e;
            } else if (n <= max_leaf) return make_leaf(b, e, box);
        }
        if (!have_split) {
            if (n <= max_leaf) return make_leaf(b, e, box);
            int ax = 0; // median split along the widest centroid axis (ties: index order)
            for (int k = 1; k < 3; ++k) if (cb.hi[k] - cb.lo[k] > cb.hi[ax] - cb.lo[ax]) ax = k;
            mid = b + n / 2;
            std::nth_element(idx.begin() + b, idx.begin() + mid, idx.begin() + e, [&](uint32_t x, uint32_t y) {
                const float cx = prims[x].c[ax], cy = prims[y].c[ax];
                return cx < cy || (cx == cy && x < y);
            });
        }
        const int32_t me = (int32_t)nodes.size();
        nodes.push_back(Tmp{});
        const int32_t l = build(b, mid, depth + 1);
        const int32_t r = build(mid, e, depth + 1);
        Tmp &t = nodes[me];
        t.box = box; t.left = l; t.right = r; t.first = 0; t.count = 0;
        return me;
    }
};

// The same tree as Builder::build(0, n, 0), built on several threads: the top levels serially down to depth `kParDepth`, every
// big range found there on a thread of its own (disjoint ranges of `idx`, a private node vector each), then spliced behind the top
// part with the indices shifted. Splits depend only on a range's own primitives, so the topology — and with it the emitted blob
// — is the serial one; only the order of the nodes in `nodes` differs, which nothing reads.
constexpr int kParDepth = 4;
int32_t build_parallel(Builder &B, uint32_t n, uint32_t serial_below = 1u << 16, uint32_t defer_above = 4096)
{
    const unsigned hw = std::thread::hardware_concurrency();
    if (n < serial_below || hw < 2) return B.build(0, n, 0);
    B.defer_depth = kParDepth; B.defer_above = defer_above;
    const int32_t root = B.build(0, n, 0);
    B.defer_depth = -1;
    const std::vector<Builder::Deferred> jobs = B.deferred;
    std::vector<Builder> subs;
    subs.reserve(jobs.size());
    for (const auto &j : jobs) { subs.emplace_back(B.prims, B.idx, (size_t)(j.e - j.b)); subs.back().max_leaf = B.max_leaf; }
    std::vector<int32_t> roots(jobs.size(), 0);
    std::vector<std::thread> th;
    for (size_t k = 0; k < jobs.size(); ++k)
        th.emplace_back([&, k] { roots[k] = subs[k].build(jobs[k].b, jobs[k].e, jobs[k].depth); });
    for (auto &t : th) t.join();
    for (size_t k = 0; k < jobs.size(); ++k) {
        const int32_t off = (int32_t)B.nodes.size();
        for (Tmp t : subs[k].nodes) {
            if (!t.count) { t.left += off; t.right += off; }
            B.nodes.push_back(t);
        }
        B.nodes[(size_t)jobs[k].node] = B.nodes[(size_t)(off + roots[k])]; // the placeholder becomes the subtree's root (children already shifted)
    }
    return root;
}

// Binary tree (tmp nodes, leaves = ranges of idx) -> blob: collapse to `width` children per node (the dynamic programme
// below), lay nodes out breadth-first, emit triangles in leaf order, compute depth and the worst-case stack need.
// octant_slots (width 8, layout BVH8O): a node's children are placed in the slot whose index names the corner of the node they sit in
// — bit k of the slot = child lies towards +axis k — so that `slot ^ (sign bits of the ray direction)` is a front-to-back order
// and the traversal needs no distance sort (the child-to-slot assignment of Ylitie, Karras & Laine, "Efficient incoherent ray
// traversal on GPUs through compressed wide BVHs", HPG 2017: greedy on the projection of the child's centre onto the slot's diagonal).
void emit_blob(const std::vector<Tmp> &tn, int32_t root, const std::vector<uint32_t> &idx, const float *verts9, const uint32_t *mats,
               uint32_t n_tris, uint32_t width, BvhBlob &out, bool octant_slots = false)
{
    struct Pending { int32_t kids[8]; int nk; }; // width <= 8; kids[c] < 0: empty slot (octant_slots leaves holes anywhere)
    std::vector<Pending> pend;
    pend.reserve(tn.size());
    // Which binary nodes become the children of a wide node: chosen by the SAH-optimal dynamic programme of Ylitie, Karras & Laine
    // (HPG 2017, §3.1) — round 1-2 opened the child of largest area until the node was full (against that rule: 1M-triangle Cornell
    // 7.60 -> 7.48 node visits per ray with 16 % fewer nodes, soup 28.92 -> 28.72).
    // cost[n][i-1] = least SAH cost of the subtree under binary node n when it may take up to i child slots of its parent (i = 1: n is
    // itself a node, or a leaf — the binary builder's leaves stay leaves, so the triangle term is a constant of the tree).
    const float c_tri = 0.6f; // a triangle test relative to a node visit
    std::vector<float> cost(tn.size() * width, 0.f);
    auto C = [&](int32_t n, uint32_t i) -> float & { return cost[(size_t)n * width + (i - 1)]; };
    auto best_split = [&](int32_t n, uint32_t j, uint32_t &kbest) { // least cost of giving j >= 2 slots to the two children of n
        float best = kInf; kbest = 1;
        for (uint32_t k = 1; k < j; ++k) { const float v = C(tn[n].left, k) + C(tn[n].right, j - k); if (v < best) { best = v; kbest = k; } }
        return best;
    };
    for (int64_t n = (int64_t)tn.size() - 1; n >= 0; --n) { // children have larger indices than their parents
        const float a = tn[n].box.area() / sah_root_area(tn[root].box);
        if (tn[n].count) { for (uint32_t i = 1; i <= width; ++i) C((int32_t)n, i) = a * c_tri * (float)tn[n].count; continue; }
        if (tn[n].left < 0 || tn[n].right < 0) continue; // (placeholder of the parallel build: never reachable)
        uint32_t k;
        C((int32_t)n, 1) = a + best_split((int32_t)n, width, k);
        for (uint32_t i = 2; i <= width; ++i) C((int32_t)n, i) = std::min(best_split((int32_t)n, i, k), C((int32_t)n, i - 1));
    }
    std::function<void(int32_t, uint32_t, Pending &)> gather = [&](int32_t n, uint32_t j, Pending &p) { // the <= j roots binary node n contributes
        if (tn[n].count || j == 1) { p.kids[p.nk++] = n; return; }
        uint32_t k;
        const float split = best_split(n, j, k);
        if (C(n, j - 1) <= split) { gather(n, j - 1, p); return; }
        gather(tn[n].left, k, p); gather(tn[n].right, j - k, p);
    };
    auto expand = [&](int32_t t) { // children of the output node made from tmp node t
        Pending p; p.nk = 0;
        for (int i = 0; i < 8; ++i) p.kids[i] = -1;
        if (tn[t].count) { p.kids[p.nk++] = t; return p; } // (root is a leaf) single child
        uint32_t k; (void)best_split(t, width, k);
        gather(tn[t].left, k, p); gather(tn[t].right, width - k, p);
        if (octant_slots && width == 8) {
            float cen[8][3], mid[3];
            Box all = Box::empty();
            for (int i = 0; i < p.nk; ++i) all.grow(tn[p.kids[i]].box);
            for (int a = 0; a < 3; ++a) mid[a] = 0.5f * (all.lo[a] + all.hi[a]);
            for (int i = 0; i < p.nk; ++i) for (int a = 0; a < 3; ++a) cen[i][a] = 0.5f * (tn[p.kids[i]].box.lo[a] + tn[p.kids[i]].box.hi[a]) - mid[a];
            int32_t placed[8]; for (int sl = 0; sl < 8; ++sl) placed[sl] = -1;
            bool done[8] = {};
            for (int round = 0; round < p.nk; ++round) { // greedy: the (child, free slot) pair of largest projection; ties: lowest child, lowest slot
                int bc = -1, bs = -1; float bv = -kInf;
                for (int i = 0; i < p.nk; ++i) {
                    if (done[i]) continue;
                    for (int sl = 0; sl < 8; ++sl) {
                        if (placed[sl] >= 0) continue;
                        const float v = (sl & 1 ? cen[i][0] : -cen[i][0]) + (sl & 2 ? cen[i][1] : -cen[i][1]) + (sl & 4 ? cen[i][2] : -cen[i][2]);
                        if (v > bv) { bv = v; bc = i; bs = sl; }
                    }
                }
                placed[bs] = p.kids[bc]; done[bc] = true;
            }
            for (int sl = 0; sl < 8; ++sl) p.kids[sl] = placed[sl];
            p.nk = 8;
        } else for (int i = p.nk; i < 8; ++i) p.kids[i] = -1;
        return p;
    };
    pend.push_back(expand(root));
    out.tris.reserve(n_tris);
    out.slots.reserve(tn.size() * width);
    const float root_area = sah_root_area(tn[root].box);
    double sah = 0.0;
    for (size_t i = 0; i < pend.size(); ++i) { // pend grows while we iterate: index i = output node i
        const Pending p = pend[i];
        BvhSlot s[8];
        for (uint32_t c = 0; c < width; ++c) { std::memset(&s[c], 0, sizeof(BvhSlot)); s[c].ref = kEmptyRef; }
        for (int c = 0; c < p.nk; ++c) {
            if (p.kids[c] < 0) continue;
            const Tmp &k = tn[p.kids[c]];
            for (int a = 0; a < 3; ++a) { s[c].lo[a] = k.box.lo[a]; s[c].hi[a] = k.box.hi[a]; }
            if (k.count) {
                const uint32_t first = (uint32_t)out.tris.size();
                for (uint32_t j = 0; j < k.count; ++j) {
                    const uint32_t id = idx[k.first + j];
                    float rows[12]; // the record's rows 0-2 are the blob's triangle
                    tri_rows(verts9 + (size_t)id * 9, id, mats ? mats[id] : 0u, rows);
                    BvhTri t; std::memcpy(&t, rows, sizeof t);
                    out.tris.push_back(t);
                }
                s[c].ref = leaf_ref(first, k.count);
            } else {
                s[c].ref = (int32_t)pend.size();
                pend.push_back(expand(p.kids[c]));
            }
            sah += sah_child_term(k.box.area(), root_area, s[c].ref);
        }
        for (uint32_t c = 0; c < width; ++c) out.slots.push_back(s[c]);
    }
    out.n_nodes = (uint32_t)pend.size();
    out.sah_cost = (float)sah;

    // ---- depth and worst-case traversal-stack need (children have larger indices than parents)
    std::vector<uint32_t> depth(out.n_nodes, 1), need(out.n_nodes, 0);
    for (int64_t i = (int64_t)out.n_nodes - 1; i >= 0; --i) {
        DepthNeed f;
        for (uint32_t c = 0; c < width; ++c) f.child(out.slots[(size_t)i * width + c].ref, depth.data(), need.data());
        depth[i] = f.depth();
        need[i] = f.need();
    }
    out.max_depth = depth[0];
    out.stack_need = need[0];
}

} // namespace

void build_bvh(const float *verts9, const uint32_t *mats, uint32_t n_tris, uint32_t width, BvhBlob &out, bool octant_slots)
{
    const auto t0 = std::chrono::steady_clock::now();
    out = BvhBlob{};
    out.width = width;
    if (n_tris == 0) return;

    std::vector<Prim> prims(n_tris);
    std::vector<uint32_t> idx(n_tris);
    for (uint32_t i = 0; i < n_tris; ++i) {
        prims[i].box = tri_box(verts9 + (size_t)i * 9, prims[i].c);
        idx[i] = i;
    }
    Builder B(prims, idx);
    const int32_t root = build_parallel(B, n_tris);
    emit_blob(B.nodes, root, idx, verts9, mats, n_tris, width, out, octant_slots);
    out.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// A binary LBVH built on the device (lbvh.hip) -> blob, in two storeys:
//   top    : the LBVH is cut where a subtree holds at most kClusterTris triangles; build_sah_over_boxes makes a binned-SAH binary tree over
//            those clusters (65 k boxes for 1M triangles; above 8192 boxes the subtrees below its top levels are built on threads: a few
//            milliseconds). Every ray crosses the top levels, and Morton splits are at their worst there (1M-triangle Cornell:
//            9.15 -> 7.9 node visits per ray).
//   bottom : inside a cluster the device's topology and boxes are kept; subtrees of at most kMaxLeaf triangles become leaves unless
//            splitting them lowers the SAH cost — blob_rules.h lbvh_leaf, the rule of Builder::build (their triangles are contiguous in
//            Morton order).
void build_bvh_from_binary(const BinaryBvh &bt, const float *verts9, const uint32_t *mats, uint32_t n_tris, uint32_t width, BvhBlob &out, bool octant_slots)
{
    const auto t0 = std::chrono::steady_clock::now();
    out = BvhBlob{};
    out.width = width;
    if (n_tris < 2 || bt.order.size() != n_tris) return;
    auto node_box = [&](int32_t c) { // (a single-triangle leaf: its padded box, exactly as the device made it)
        return c >= 0 ? Box::of(&bt.box[(size_t)c * 6]) : tri_box(verts9 + (size_t)bt.order[(uint32_t)~c] * 9);
    };
    auto node_count = [&](int32_t c) { return c >= 0 ? bt.last[c] - bt.first[c] + 1 : 1u; };

    // ---- cut: cluster roots, in Morton order
    std::vector<int32_t> clusters;
    {
        std::vector<int32_t> st{ 0 };
        while (!st.empty()) {
            const int32_t c = st.back(); st.pop_back();
            if (c < 0 || node_count(c) <= kClusterTris) clusters.push_back(c);
            else { st.push_back(bt.right[c]); st.push_back(bt.left[c]); }
        }
    }
    // ---- top storey: binned SAH over the cluster boxes, one cluster per leaf
    const uint32_t nc = (uint32_t)clusters.size();
    std::vector<float> cbox((size_t)nc * 6), top_box;
    for (uint32_t i = 0; i < nc; ++i) {
        const Box b = node_box(clusters[i]);
        for (int k = 0; k < 3; ++k) { cbox[(size_t)i * 6 + k] = b.lo[k]; cbox[(size_t)i * 6 + 3 + k] = b.hi[k]; }
    }
    std::vector<int32_t> top_left, top_right;
    int32_t top_root = 0;
    build_sah_over_boxes(cbox.data(), nc, top_left, top_right, top_box, top_root);
    // as tmp nodes: the top's inner nodes keep their numbers (parents before children), cluster i follows them at n_top + i, and the
    // bottom storey goes behind — so children have larger indices than their parents, which emit_blob relies on
    const int32_t n_top = (int32_t)top_left.size();
    auto at = [&](int32_t c) { return c < 0 ? n_top + ~c : c; };
    std::vector<Tmp> tn((size_t)n_top + nc);
    tn.reserve(tn.size() + (size_t)n_tris * 2);
    for (int32_t i = 0; i < n_top; ++i) tn[i] = Tmp{ Box::of(&top_box[(size_t)i * 6]), at(top_left[i]), at(top_right[i]), 0u, 0u };
    const int32_t root = at(top_root);

    // ---- bottom storey: every cluster's place is filled by its LBVH subtree (iterative: deep chains stay off the C stack)
    struct Work { int32_t node; int32_t at; }; // convert LBVH node `node` into tn[at]
    std::vector<Work> work;
    for (uint32_t i = 0; i < nc; ++i) work.push_back({ clusters[i], n_top + (int32_t)i });
    while (!work.empty()) {
        const Work w = work.back(); work.pop_back();
        Tmp t; t.left = t.right = -1; t.first = 0; t.count = 0;
        t.box = node_box(w.node);
        if (w.node >= 0) {
            const int32_t l = bt.left[w.node], r = bt.right[w.node];
            const uint32_t cnt = node_count(w.node);
            if (cnt <= kMaxLeaf && lbvh_leaf(cnt, t.box.area(), node_count(l), node_box(l).area(), node_count(r), node_box(r).area())) { // (asked first: a bigger node's child boxes stay unmade)
                t.first = bt.first[w.node]; t.count = cnt;
            }
            else {
                t.left = (int32_t)tn.size(); t.right = t.left + 1;
                tn.push_back(Tmp{}); tn.push_back(Tmp{});
                work.push_back({ l, t.left });
                work.push_back({ r, t.right });
            }
        } else { t.first = (uint32_t)~w.node; t.count = 1; }
        tn[w.at] = t;
    }
    const auto t1 = std::chrono::steady_clock::now();
    emit_blob(tn, root, bt.order, verts9, mats, n_tris, width, out, octant_slots);
    if (getenv("PTRT_TIMING")) // developer aid
        fprintf(stderr, "ptrt commit: lbvh device %.2f ms, cut + SAH top + conversion %.2f ms, emit_blob %.2f ms\n", bt.device_ms,
                std::chrono::duration<double, std::milli>(t1 - t0).count(), std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count());
    out.build_ms = bt.device_ms + std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

void build_sah_over_boxes(const float *boxes6, uint32_t n, std::vector<int32_t> &left, std::vector<int32_t> &right, std::vector<float> &node_boxes6, int32_t &root)
{
    std::vector<Prim> prims(n);
    std::vector<uint32_t> idx(n);
    for (uint32_t i = 0; i < n; ++i) {
        prims[i].box = Box::of(boxes6 + (size_t)i * 6);
        for (int k = 0; k < 3; ++k) prims[i].c[k] = 0.5f * (prims[i].box.lo[k] + prims[i].box.hi[k]);
        idx[i] = i;
    }
    Builder b(prims, idx);
    b.max_leaf = 1;
    const int32_t r = build_parallel(b, n, 8192, 256);
    // internal Tmp nodes -> compact internal numbering; leaves -> ~box index
    std::vector<int32_t> number(b.nodes.size(), -1);
    int32_t n_int = 0;
    for (size_t i = 0; i < b.nodes.size(); ++i) if (!b.nodes[i].count) number[i] = n_int++;
    auto ref = [&](int32_t t) { return b.nodes[t].count ? ~(int32_t)idx[b.nodes[t].first] : number[t]; };
    left.assign(n_int, 0); right.assign(n_int, 0); node_boxes6.assign((size_t)n_int * 6, 0.f);
    for (size_t i = 0; i < b.nodes.size(); ++i) {
        if (b.nodes[i].count) continue;
        const int32_t k = number[i];
        left[k] = ref(b.nodes[i].left); right[k] = ref(b.nodes[i].right);
        for (int a = 0; a < 3; ++a) { node_boxes6[(size_t)k * 6 + a] = b.nodes[i].box.lo[a]; node_boxes6[(size_t)k * 6 + 3 + a] = b.nodes[i].box.hi[a]; }
    }
    root = ref(r);
}

// ---- BVH4Q / BVH8Q: a width-4 / width-8 blob repacked into 64- / 128-byte nodes (layouts 68 / 72, 73), child boxes quantised to 8
// bits per coordinate by blob_rules.h quantize_node, the text the GPU builder and the refit run on the device
template <int N>
static void quantize_nodes(const BvhBlob &in, std::vector<uint8_t> &out)
{
    constexpr size_t kStride = N == 4 ? 64 : 128;
    out.assign((size_t)in.n_nodes * kStride, 0);
    auto range = [&](uint32_t i0, uint32_t i1) { // nodes are independent of one another
        for (uint32_t i = i0; i < i1; ++i) {
            const BvhSlot *s = &in.slots[(size_t)i * N];
            bool used[N];
            uint32_t w[kStride / 4] = {};
            for (int c = 0; c < N; ++c) { used[c] = s[c].ref != kEmptyRef; w[4 + c] = (uint32_t)s[c].ref; }
            quantize_node<N>(s, used, w);
            std::memcpy(&out[(size_t)i * kStride], w, kStride);
        }
    };
    const uint32_t nt = in.n_nodes < (1u << 15) ? 1u : std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    if (nt == 1) { range(0, in.n_nodes); return; }
    std::vector<std::thread> th;
    for (uint32_t t = 0; t < nt; ++t) th.emplace_back(range, (uint32_t)((uint64_t)in.n_nodes * t / nt), (uint32_t)((uint64_t)in.n_nodes * (t + 1) / nt));
    for (auto &t : th) t.join();
}

void quantize_bvh4(const BvhBlob &in, std::vector<uint8_t> &out) { quantize_nodes<4>(in, out); }
void quantize_bvh8(const BvhBlob &in, std::vector<uint8_t> &out) { quantize_nodes<8>(in, out); }

} // namespace ptrt
