// pipeline_ref.cpp — pathtracing_amd/csrc/pipeline.h as plain C, for tests/pipeline_checker.py. No rule of its own: every field is what
// the header's decode or one of its members returns.
#include "../../pathtracing_amd/csrc/pipeline.h"

using namespace ptrt;

extern "C" {

struct pr_pipeline {
    int32_t status;                 // pt_status of the decode; != PT_OK: only `message` is meaningful besides
    const char *message;            // the refusal's text (static storage), NULL when accepted
    uint32_t forced;
    uint32_t profile, count, split, bucket, nee, env;
    int32_t shade, fuse;
    uint32_t full_state, resolves_sky, instrumented;
    uint32_t single_loop[2];        // [probing]
    uint32_t generate_mode[2];      // [dense]
    int32_t kernel_for[4][3];       // [choice 0..3][probe iteration: none, 2, 3]
};

void pr_decode(uint32_t flags, uint32_t tuned_kernel, int has_env, int has_specular, pr_pipeline *out)
{
    const PipelineDecode d = decode_pipeline(flags, tuned_kernel, has_env != 0, has_specular != 0);
    const Pipeline &p = d.pipeline;
    *out = pr_pipeline{};
    out->status = d.status; out->message = d.message;
    if (d.status != PT_OK) return;
    out->forced = p.forced;
    out->profile = p.profile; out->count = p.count; out->split = p.split; out->bucket = p.bucket; out->nee = p.nee; out->env = p.env;
    out->shade = p.shade; out->fuse = p.fuse();
    out->full_state = p.full_state(); out->resolves_sky = p.resolves_sky(); out->instrumented = p.instrumented();
    static const uint32_t probe_iterations[3] = { 0u, 2u, 3u };
    for (int b = 0; b < 2; ++b) { out->single_loop[b] = p.single_loop(b != 0); out->generate_mode[b] = p.generate_mode(b != 0); }
    for (uint32_t choice = 0; choice < 4; ++choice)
        for (int i = 0; i < 3; ++i) out->kernel_for[choice][i] = p.kernel_for(choice, probe_iterations[i]);
}

int pr_forces_compact(uint32_t flags, int repack_sticky, uint32_t samples_per_stream)
{
    return decode_pipeline(flags, 0u, false, false).pipeline.forces_compact(repack_sticky != 0, samples_per_stream);
}

int pr_extend_instantiated(int kernel, int fuse, int count, int nee, int env) { return extend_instantiated(kernel, fuse, count != 0, nee != 0, env != 0); }

uint32_t pr_extend_kernel_first(void) { return kExtendKernelFirst; }
uint32_t pr_extend_kernel_last(void) { return kExtendKernelLast; }

}
