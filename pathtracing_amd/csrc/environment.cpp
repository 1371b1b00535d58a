// environment.cpp — pt_scene_set_environment, pt_scene_environment_info, pt_scene_environment_read: validation, the sampling table of
// docs/SPEC.md §11 (built in double, stored as the kernels read it), its upload and its read-back.
#include "scene.h"
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>

using namespace ptrt;

namespace {

// §11: the 1-norm of the unit direction of the centre of texel (i, j), in double
double centre_norm1(uint32_t i, uint32_t j, uint32_t n)
{
    const double u = (double)(2u * i + 1u) / (double)n - 1.0, v = (double)(2u * j + 1u) / (double)n - 1.0;
    const double z = (1.0 - std::fabs(u)) - std::fabs(v);
    double x = u, y = v;
    if (z < 0.0) { x = (1.0 - std::fabs(v)) * std::copysign(1.0, u); y = (1.0 - std::fabs(u)) * std::copysign(1.0, v); }
    const double len = std::sqrt((x * x + y * y) + z * z);
    return (std::fabs(x / len) + std::fabs(y / len)) + std::fabs(z / len);
}

} // namespace

pt_status Environment::set(pt_context *c, const float *rgb, uint32_t n)
{
    if ((rgb == nullptr) != (n == 0u)) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_scene_set_environment: rgb and n must both be given, or NULL and 0 to remove the environment");
    if (n > 2048u) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_scene_set_environment: n = %u, the map is at most 2048 x 2048 texels", n);
    if (c) HIP_TRY(c, hipSetDevice(c->device));
    if (n == 0u) { *this = Environment{}; return PT_OK; }
    const size_t nn = (size_t)n * n;
    for (size_t k = 0; k < nn * 3; ++k)
        if (!(std::isfinite(rgb[k]) && rgb[k] >= 0.0f)) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_scene_set_environment: component %llu is negative or not finite", (unsigned long long)k);
    // w_k = (r + g + b) * sc^3, the row sums and their total, all in row-major order
    std::vector<double> w(nn), R(n);
    double total = 0.0;
    for (uint32_t j = 0; j < n; ++j) {
        double row = 0.0;
        for (uint32_t i = 0; i < n; ++i) {
            const float *t = rgb + ((size_t)j * n + i) * 3;
            const double sc = centre_norm1(i, j, n);
            const double wk = ((double)t[0] + (double)t[1] + (double)t[2]) * ((sc * sc) * sc);
            w[(size_t)j * n + i] = wk; row += wk;
        }
        R[j] = row; total += row;
    }
    Environment e;
    e.n_ = n; e.lit_ = total > 0.0; e.total_ = total;
    e.texels_.resize(nn * 4); e.mcdf_.resize(n); e.ccdf_.resize(nn);
    const double scale = (double)n * (double)n / 4.0;
    double S = 0.0;
    for (uint32_t j = 0; j < n; ++j) {
        S += R[j];
        e.mcdf_[j] = (e.lit_ && j + 1u < n) ? (float)(S / total) : 1.0f;
        double run = 0.0;
        for (uint32_t i = 0; i < n; ++i) {
            const size_t k = (size_t)j * n + i;
            run += w[k];
            e.ccdf_[k] = (e.lit_ && R[j] > 0.0 && i + 1u < n) ? (float)(run / R[j]) : 1.0f;
            e.texels_[k * 4] = rgb[k * 3]; e.texels_[k * 4 + 1] = rgb[k * 3 + 1]; e.texels_[k * 4 + 2] = rgb[k * 3 + 2];
            e.texels_[k * 4 + 3] = e.lit_ ? (float)(w[k] / total * scale) : 0.0f;
        }
    }
    if (c) { // new buffers, filled before they replace the old ones
        hipStream_t q = c->stream;
        HIP_TRY(c, e.d_texels.ensure(nn)); HIP_TRY(c, e.d_mcdf.ensure(n)); HIP_TRY(c, e.d_ccdf.ensure(nn));
        HIP_TRY(c, hipMemcpyAsync(e.d_texels.p, e.texels_.data(), nn * 4 * sizeof(float), hipMemcpyHostToDevice, q));
        HIP_TRY(c, hipMemcpyAsync(e.d_mcdf.p, e.mcdf_.data(), n * sizeof(float), hipMemcpyHostToDevice, q));
        HIP_TRY(c, hipMemcpyAsync(e.d_ccdf.p, e.ccdf_.data(), nn * sizeof(float), hipMemcpyHostToDevice, q));
        HIP_TRY(c, hipStreamSynchronize(q));
    }
    *this = std::move(e);
    return PT_OK;
}

extern "C" {

pt_status pt_scene_set_environment(pt_scene *s, const float *rgb, uint32_t n)
{
    if (!s) return fail(nullptr, PT_ERR_INVALID_ARGUMENT, "scene is NULL");
    return s->env.set(s->ctx, rgb, n);
}

pt_status pt_scene_environment_info(const pt_scene *s, pt_environment_info *out)
{
    if (!s || !out) return fail(s ? s->ctx : nullptr, PT_ERR_INVALID_ARGUMENT, "pt_scene_environment_info: NULL argument");
    out->n = s->env.n(); out->lit = s->env.lit() ? 1u : 0u; out->device_bytes = s->env.device_bytes(); out->total = s->env.total();
    return PT_OK;
}

pt_status pt_scene_environment_read(const pt_scene *s, float *texels4, float *mcdf, float *ccdf, uint64_t n_texels)
{
    if (!s || !texels4 || !mcdf || !ccdf) return fail(s ? s->ctx : nullptr, PT_ERR_INVALID_ARGUMENT, "pt_scene_environment_read: NULL argument");
    const Environment &e = s->env;
    if (!e.present()) return fail(s->ctx, PT_ERR_INVALID_ARGUMENT, "pt_scene_environment_read: the scene has no environment");
    const uint64_t nn = (uint64_t)e.n() * e.n();
    if (n_texels < nn) return fail(s->ctx, PT_ERR_INVALID_ARGUMENT, "buffer too small: need %llu texels", (unsigned long long)nn);
    std::memcpy(texels4, e.texels4().data(), nn * 4 * sizeof(float));
    std::memcpy(mcdf, e.mcdf().data(), e.n() * sizeof(float));
    std::memcpy(ccdf, e.ccdf().data(), nn * sizeof(float));
    return PT_OK;
}

} // extern "C"
