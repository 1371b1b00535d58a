// environment.h — the one owner of a scene's environment map (pt_scene_set_environment, docs/SPEC.md §11): the sampling table on the
// host, exactly as the kernels read it, and its device copy when the scene has a context. Private to environment.cpp (the three public
// calls), scene.h (the member) and frame.cpp (the frame's EnvArgs).
#pragma once
#include "context.h"
#include <vector>

namespace ptrt {

class Environment {
public:
    // Validates (1 <= n <= 2048, every component finite and >= 0; rgb == NULL && n == 0 removes), builds the table in double, uploads
    // it on the context's stream and waits (c == NULL: host table only). A refused or failed call leaves the old environment in place.
    pt_status set(pt_context *c, const float *rgb, uint32_t n);
    bool present() const { return n_ != 0u; }
    uint32_t n() const { return n_; }
    bool lit() const { return lit_; }
    double total() const { return total_; }
    uint64_t device_bytes() const { return (d_texels.n * 4u + d_mcdf.n + d_ccdf.n) * sizeof(float); }
    const std::vector<float> &texels4() const { return texels_; } // n * n * 4
    const std::vector<float> &mcdf() const { return mcdf_; }      // n
    const std::vector<float> &ccdf() const { return ccdf_; }      // n * n
    EnvArgs args(float psel) const { return EnvArgs{ d_texels.p, d_mcdf.p, d_ccdf.p, n_, (float)n_, 2.0f / (float)n_, lit_ ? 1u : 0u, psel }; }

private:
    uint32_t n_ = 0;
    bool lit_ = false;
    double total_ = 0.0;
    std::vector<float> texels_, mcdf_, ccdf_;
    DevBuf<float4> d_texels;
    DevBuf<float> d_mcdf, d_ccdf;
};

} // namespace ptrt
