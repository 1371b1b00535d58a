// denoise.hip — pt_denoise (docs/SPEC.md §8) on gfx950: the first-hit guide buffers and the edge-aware à-trous filter.
//
//   k_guide_index   : original triangle id -> blob index, from every record's row 0 .w (once per commit; query.cpp caches it in the scene)
//   k_guide_rays    : the unjittered §3 camera ray of every pixel, as a pt_trace_rays record; kernels.hip's k_trace then finds the hits
//   k_guide_resolve : {t, prim id} -> g0 = (front-facing normal, t), g1 = (albedo, prim id bits): triangles read the record's shading
//                     row, spheres the 1/r of sph_mat
//   k_guide_resolve_tex : the same on a textured scene (docs/SPEC.md §13): g1.rgb = albedo * texel of a triangle hit, the texel looked up
//                     at the hit record's (u, v); a kernel of its own, so that k_guide_resolve keeps its code
//   k_atrous<EDGE>  : one filter pass, 64x4 workgroups as k_assemble: a wave covers 64 pixels of one row, so each of a tap's three rows
//                     (colour, g0, g1) is one coalesced 1 KiB load; the centre pixel's colour and guides stay in registers, one division
//                     per tap (the four edge-stop denominators multiplied first)
// Op order follows §8 exactly (explicit fma, -ffp-contract=off, IEEE division): tests/denoise_ref/ restates it bit for bit.
#include "ptrt_internal.h"
#include "pt_device.h"
#include "texture_device.h"
#include "denoise.h"
#include <cstring>

using namespace ptd;

namespace ptrt {

__global__ void __launch_bounds__(kBlock) k_guide_index(const float4 *__restrict__ tris, uint32_t n_tris, uint32_t *__restrict__ blob_of)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= n_tris) return;
    const uint32_t id = __float_as_uint(tris[(size_t)j * 4].w);
    if (id < n_tris) blob_of[id] = j;
}

__global__ void __launch_bounds__(kBlock) k_guide_rays(Camera cam, uint32_t w, uint32_t h, float4 *__restrict__ rays)
{
    const uint32_t x = blockIdx.x * 64u + threadIdx.x, y = blockIdx.y * 4u + threadIdx.y;
    if (x >= w || y >= h) return;
    V3 o, d;
    camera_ray(cam, x, y, 0u, o, d); // cam.jitter == 0: jx = jy = 0.5f, the key is not read
    const size_t i = (size_t)y * w + x;
    rays[2 * i] = make_float4(o.x, o.y, o.z, __builtin_inff());
    rays[2 * i + 1] = make_float4(d.x, d.y, d.z, 0.0f);
}

__global__ void __launch_bounds__(kBlock) k_guide_resolve(DeviceScene sc, const uint32_t *__restrict__ blob_of, const float4 *__restrict__ rays,
                                                          const float4 *__restrict__ hits, uint32_t n, float4 *__restrict__ g0, float4 *__restrict__ g1)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float4 hit = hits[i];
    const uint32_t id = __float_as_uint(hit.y);
    if (id == PT_MISS) {
        g0[i] = make_float4(0.0f, 0.0f, 0.0f, __builtin_inff());
        g1[i] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(PT_MISS));
        return;
    }
    const V3 d = xyz(rays[2 * (size_t)i + 1]);
    V3 ng;
    uint32_t mat;
    if (id < sc.n_tris) { // the shading row normalize(cross(e1, e2)) | material of the triangle's record
        const float4 row = sc.tris[(size_t)blob_of[id] * 4 + 3];
        ng = xyz(row);
        mat = __float_as_uint(row.w);
    } else {
        const uint32_t j = id - sc.n_tris;
        const V3 o = xyz(rays[2 * (size_t)i]), c = xyz(sc.spheres[j]);
        const uint2 sm = sc.sph_mat[j];
        const float inv_r = __uint_as_float(sm.y);
        const V3 P = madd(hit.x, d, o);
        ng = V3{ (P.x - c.x) * inv_r, (P.y - c.y) * inv_r, (P.z - c.z) * inv_r };
        mat = sm.x;
    }
    const V3 nf = dot(ng, d) < 0.0f ? ng : neg(ng);
    const float4 m0 = sc.mats[(size_t)mat * 3]; // kind, albedo.rgb
    g0[i] = make_float4(nf.x, nf.y, nf.z, hit.x);
    g1[i] = make_float4(m0.y, m0.z, m0.w, hit.y);
}

__global__ void __launch_bounds__(kBlock) k_guide_resolve_tex(DeviceScene sc, const uint32_t *__restrict__ blob_of, const float4 *__restrict__ rays,
                                                              const float4 *__restrict__ hits, uint32_t n, float4 *__restrict__ g0, float4 *__restrict__ g1,
                                                              TexArgs tex)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float4 hit = hits[i];
    const uint32_t id = __float_as_uint(hit.y);
    if (id == PT_MISS) {
        g0[i] = make_float4(0.0f, 0.0f, 0.0f, __builtin_inff());
        g1[i] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(PT_MISS));
        return;
    }
    const V3 d = xyz(rays[2 * (size_t)i + 1]);
    V3 ng, texel = v3(1.0f, 1.0f, 1.0f);
    uint32_t mat;
    if (id < sc.n_tris) {
        const uint32_t blob = blob_of[id];
        const float4 row = sc.tris[(size_t)blob * 4 + 3];
        ng = xyz(row);
        mat = __float_as_uint(row.w);
        texel = tex_of_hit(tex, blob, hit.z, hit.w); // §13: (u, v) of the guide ray's hit record
    } else {
        const uint32_t j = id - sc.n_tris;
        const V3 o = xyz(rays[2 * (size_t)i]), c = xyz(sc.spheres[j]);
        const uint2 sm = sc.sph_mat[j];
        const float inv_r = __uint_as_float(sm.y);
        const V3 P = madd(hit.x, d, o);
        ng = V3{ (P.x - c.x) * inv_r, (P.y - c.y) * inv_r, (P.z - c.z) * inv_r };
        mat = sm.x;
    }
    const V3 nf = dot(ng, d) < 0.0f ? ng : neg(ng);
    const float4 m0 = sc.mats[(size_t)mat * 3]; // kind, albedo.rgb
    g0[i] = make_float4(nf.x, nf.y, nf.z, hit.x);
    g1[i] = make_float4(m0.y * texel.x, m0.z * texel.y, m0.w * texel.z, hit.y);
}

PT_DEV float edge_d(float x) { return fma_(x, fma_(x, 0.5f, 1.0f), 1.0f); } // ~e^x near 0, no transcendental
PT_DEV float dot4_3(float4 a, float4 b) { return fma_(a.z, b.z, fma_(a.y, b.y, a.x * b.x)); }
PT_DEV float b3(int k) { return k == 0 ? 0.375f : (k == 1 || k == -1) ? 0.25f : 0.0625f; }
PT_DEV float clamp_scale(float v) { return fmin_(fmax_(v, 0x1p-149f), 3.40282347e+38f); } // §8.2: an inverse scale is never 0 or +inf

template <bool EDGE>
__global__ void __launch_bounds__(kBlock) k_atrous(AtrousParams p, const float4 *__restrict__ src, const float4 *__restrict__ g0,
                                                   const float4 *__restrict__ g1, float4 *__restrict__ dst)
{
    const int x = (int)(blockIdx.x * 64u + threadIdx.x), y = (int)(blockIdx.y * 4u + threadIdx.y);
    const int w = (int)p.width, h = (int)p.height;
    if (x >= w || y >= h) return;
    const int s = 1 << p.pass;
    const size_t ip = (size_t)y * w + x;
    const float4 cp = src[ip], np = g0[ip], ap = g1[ip];
    const bool miss_p = __float_as_uint(ap.w) == PT_MISS;
    const float iz = clamp_scale(1.0f / ((p.sigma_z * np.w) * (float)s)); // (used only when p is a hit)
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + dy * s;
        if (qy < 0 || qy >= h) continue; // uniform over the wave (a wave is one row segment)
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * s;
            if (qx < 0 || qx >= w) continue;
            const size_t iq = (size_t)qy * w + qx;
            const float4 aq = g1[iq];
            if (miss_p != (__float_as_uint(aq.w) == PT_MISS)) continue;
            const float4 cq = src[iq];
            float wt = b3(dx) * b3(dy);
            if (EDGE) {
                const float4 dc = make_float4(cp.x - cq.x, cp.y - cq.y, cp.z - cq.z, 0.0f);
                const float xc = dot4_3(dc, dc) * p.ic_i;
                float xn = 0.0f, xz = 0.0f, xa = 0.0f;
                if (!miss_p) {
                    const float4 nq = g0[iq];
                    xn = fmax_(0.0f, 1.0f - dot4_3(np, nq)) * p.inv_sn;
                    xz = __builtin_fabsf(nq.w - np.w) * iz;
                    const float4 da = make_float4(ap.x - aq.x, ap.y - aq.y, ap.z - aq.z, 0.0f);
                    xa = dot4_3(da, da) * p.ia;
                }
                wt = wt / (((edge_d(xc) * edge_d(xn)) * edge_d(xz)) * edge_d(xa));
            }
            sw = sw + wt;
            sr = fma_(wt, cq.x, sr); sg = fma_(wt, cq.y, sg); sb = fma_(wt, cq.z, sb);
        }
    }
    // The centre tap usually gives sw >= 0.140625, but its x_n = max(0, 1 - |n|^2) * inv_sn is not 0 where |n|^2 < 1 in f32, so with a
    // huge inv_sn every weight can vanish: then 1/sw overflows and the pixel is kept as it is (§8.2).
    const float r = 1.0f / sw;
    dst[ip] = r <= 3.40282347e+38f ? make_float4(sr * r, sg * r, sb * r, cp.w) : cp;
}

// ================================================================================================ launchers
static inline dim3 rows_grid(uint32_t w, uint32_t h) { return dim3((w + 63u) / 64u, (h + 3u) / 4u, 1u); }

hipError_t launch_guide_index(hipStream_t s, const float4 *tris, uint32_t n_tris, uint32_t *blob_of)
{
    if (!n_tris) return hipSuccess;
    hipLaunchKernelGGL(k_guide_index, dim3((n_tris + kBlock - 1u) / kBlock), dim3(kBlock), 0, s, tris, n_tris, blob_of);
    return hipGetLastError();
}

hipError_t launch_guide_rays(hipStream_t s, const pt_camera &cam, uint32_t w, uint32_t h, float4 *rays)
{
    static_assert(sizeof(Camera) == sizeof(pt_camera), "camera layout");
    Camera c;
    std::memcpy(&c, &cam, sizeof c);
    c.jitter = 0u;
    hipLaunchKernelGGL(k_guide_rays, rows_grid(w, h), dim3(64, 4, 1), 0, s, c, w, h, rays);
    return hipGetLastError();
}

hipError_t launch_guide_resolve(hipStream_t s, const DeviceScene &sc, const uint32_t *blob_of, const float4 *rays, const float4 *hits,
                                uint32_t n, float4 *g0, float4 *g1, const TexArgs *tex)
{
    if (tex) hipLaunchKernelGGL(k_guide_resolve_tex, dim3((n + kBlock - 1u) / kBlock), dim3(kBlock), 0, s, sc, blob_of, rays, hits, n, g0, g1, *tex);
    else hipLaunchKernelGGL(k_guide_resolve, dim3((n + kBlock - 1u) / kBlock), dim3(kBlock), 0, s, sc, blob_of, rays, hits, n, g0, g1);
    return hipGetLastError();
}

hipError_t launch_atrous(hipStream_t s, const AtrousParams &p, const float4 *src, const float4 *g0, const float4 *g1, float4 *dst)
{
    if (p.edge_stops) hipLaunchKernelGGL(k_atrous<true>, rows_grid(p.width, p.height), dim3(64, 4, 1), 0, s, p, src, g0, g1, dst);
    else hipLaunchKernelGGL(k_atrous<false>, rows_grid(p.width, p.height), dim3(64, 4, 1), 0, s, p, src, g0, g1, dst);
    return hipGetLastError();
}

} // namespace ptrt
