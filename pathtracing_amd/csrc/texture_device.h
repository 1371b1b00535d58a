// texture_device.h — gfx950 device functions of the albedo textures (docs/SPEC.md §13), op for op: the coordinate of a triangle hit from its
// barycentrics, repeat wrap by floorf, the nearest and the bilinear lookup. Shared by the textured instantiations of k_extend (kernels.hip
// shade_one<.., TEX>) and by k_guide_resolve_tex (denoise.hip); tests/tex_ref/ restates it in plain C.
#pragma once
#include "ptrt_internal.h"
#include "pt_device.h"

namespace ptrt {

// floorf as one v_floor_f32 (exact, like the host's)
PT_DEV float tex_floor(float x) { return __builtin_floorf(x); }

// §13 "Bilinear": the two texel indices and the weight along one axis of n texels, from the wrapped coordinate f in [0, 1]. The final
// unsigned min changes no index of a finite coordinate (both are in [0, n - 1] by then) and keeps a non-finite one inside the texture.
PT_DEV void tex_axis(float f, uint32_t n, uint32_t &i0, uint32_t &i1, float &w)
{
    const float xf = ptd::fma_(f, (float)n, -0.5f), x0f = tex_floor(xf);
    w = xf - x0f;
    int a = (int)x0f, b = a + 1;
    if (a < 0) a += (int)n;
    if (b >= (int)n) b -= (int)n;
    i0 = min((uint32_t)a, n - 1u); i1 = min((uint32_t)b, n - 1u);
}

// §13: the texel of texture record `ds` = {first texel, width, height, flags} at (s, t)
PT_DEV ptd::V3 tex_lookup(const float4 *__restrict__ texels, uint4 ds, float s, float t)
{
    const float fs = s - tex_floor(s), ft = t - tex_floor(t);
    const float4 *__restrict__ base = texels + (size_t)ds.x;
    const uint32_t W = ds.y, H = ds.z;
    if (ds.w & PT_TEXTURE_NEAREST) {
        const int x = (int)tex_floor(fs * (float)W), y = (int)tex_floor(ft * (float)H);
        const uint32_t xi = min((uint32_t)max(x, 0), W - 1u), yi = min((uint32_t)max(y, 0), H - 1u);
        return ptd::xyz(base[(size_t)yi * W + xi]);
    }
    uint32_t x0, x1, y0, y1;
    float fx, fy;
    tex_axis(fs, W, x0, x1, fx); tex_axis(ft, H, y0, y1, fy);
    // the four texels are requested together: none of the addresses depends on another's data
    float4 a = base[(size_t)y0 * W + x0], b = base[(size_t)y0 * W + x1], p = base[(size_t)y1 * W + x0], q = base[(size_t)y1 * W + x1];
    asm volatile("" : "+v"(a.x), "+v"(b.x), "+v"(p.x), "+v"(q.x));
    const float tx = ptd::fma_(fx, b.x - a.x, a.x), bx = ptd::fma_(fx, q.x - p.x, p.x);
    const float ty = ptd::fma_(fx, b.y - a.y, a.y), by = ptd::fma_(fx, q.y - p.y, p.y);
    const float tz = ptd::fma_(fx, b.z - a.z, a.z), bz = ptd::fma_(fx, q.z - p.z, p.z);
    return ptd::v3(ptd::fma_(fy, bx - tx, tx), ptd::fma_(fy, by - ty, ty), ptd::fma_(fy, bz - tz, tz));
}

// §13 "Coordinate" and the lookup for a hit of blob triangle `blob` with barycentrics (u, v): the texel, or (1, 1, 1) — the factor that
// changes no albedo — when the triangle's material is bound to no texture.
PT_DEV ptd::V3 tex_of_hit(const TexArgs &ta, uint32_t blob, float u, float v)
{
    const float4 q0 = ta.uv[(size_t)blob * 2], q1 = ta.uv[(size_t)blob * 2 + 1];
    const uint32_t di = __float_as_uint(q1.z);
    if (di >= ta.n_desc) return ptd::v3(1.0f, 1.0f, 1.0f); // PT_NO_TEXTURE
    const uint4 ds = ta.desc[di];
    const float w0 = (1.0f - u) - v;
    const float s = ptd::fma_(v, q1.x, ptd::fma_(u, q0.z, w0 * q0.x)), t = ptd::fma_(v, q1.y, ptd::fma_(u, q0.w, w0 * q0.y));
    return tex_lookup(ta.texels, ds, s, t);
}

} // namespace ptrt
