// refit.h — pt_scene_update_triangles on the device (refit.hip): new vertices into a committed tree whose topology and leaf assignment
// stay, docs/SPEC.md §4.3. scene.cpp owns the buffers and calls these in order: stage (device input), triangles, levels deepest first, SAH.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <vector>

namespace ptrt {

// Level lists of a committed tree, from its refs (n_nodes x fan, node-major, any node memory order; root = node 0): `list` holds the node
// indices level by level, deepest level first; level l is list[off[l] .. off[l+1]). Fails (false) unless the refs form a tree whose
// inner refs are < n_nodes and whose leaf ranges lie inside n_tris — the kernels index with them unchecked.
bool refit_levels(const int32_t *refs, uint32_t n_nodes, uint32_t fan, uint32_t n_tris, std::vector<uint32_t> &list, std::vector<uint32_t> &off);

// Device input: copy n_floats from `in` to `out` and set *bad (zeroed by the caller) if any of them is not finite.
hipError_t launch_refit_stage(hipStream_t s, const float *in, float *out, uint64_t n_floats, uint32_t *bad);
// Pass 1, every blob triangle j (its original id = record row 0 .w): the 64-byte record {v0|id, e1|mat, e2|0, normalize(cross(e1,e2))|mat}
// rewritten from verts9 in the op order of docs/SPEC.md §0 (material and id words kept), and its padded box (§4.1) into tbox[6 j].
hipError_t launch_refit_tris(hipStream_t s, const float *verts9, float4 *rec, uint32_t n_tris, float *tbox);
// Pass 2, one level: every listed node's child boxes (leaf child: union of its triangles' tbox; inner child: nbox of that node) are written
// as f32 slots (layouts 2, 4) or re-quantised (68, 72, 73; refs and slot order kept), their union into nbox[6 i], their areas into
// carea[fan * i + c]. layout: PT_BVH_WIDTH_2 / _4 / _4Q / _8Q / _8O.
hipError_t launch_refit_level(hipStream_t s, uint32_t layout, void *nodes, const uint32_t *list, uint32_t count, const float *tbox,
                              float *nbox, float *carea);
// After the last level: the builder's SAH cost (bvh_build.cpp emit_blob) of the refitted f32 boxes, into *out. partial: refit_sah_blocks()
// doubles of scratch.
uint32_t refit_sah_blocks(uint32_t n_nodes);
hipError_t launch_refit_sah(hipStream_t s, uint32_t layout, const void *nodes, uint32_t n_nodes, const float *carea, const float *nbox,
                            double *partial, double *out);

} // namespace ptrt
