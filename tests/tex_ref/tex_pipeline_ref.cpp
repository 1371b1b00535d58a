// tex_pipeline_ref.cpp — the texture parameter of pathtracing_amd/csrc/pipeline.h as plain C, for tests/tex_checker.py. No rule of its
// own: every field is what the header's decode or one of its members returns. tp_decode passes has_textures, tp_decode_default leaves the
// argument out (the call every frame made before textures existed).
#include "../../pathtracing_amd/csrc/pipeline.h"

using namespace ptrt;

extern "C" {

struct tp_pipeline {
    int32_t status;
    const char *message;            // the refusal's text (static storage), NULL when accepted
    uint32_t forced;
    uint32_t profile, count, split, bucket, nee, env, lens, sph, tex;
    int32_t shade, fuse;
    uint32_t full_state, resolves_sky, instrumented;
    uint32_t single_loop[2];        // [probing]
    uint32_t generate_mode[2];      // [dense]
    int32_t kernel_for[4][3];       // [choice 0..3][probe iteration: none, 2, 3]
};

static void fill(const PipelineDecode &d, tp_pipeline *out)
{
    const Pipeline &p = d.pipeline;
    *out = tp_pipeline{};
    out->status = d.status; out->message = d.message;
    if (d.status != PT_OK) return;
    out->forced = p.forced;
    out->profile = p.profile; out->count = p.count; out->split = p.split; out->bucket = p.bucket; out->nee = p.nee; out->env = p.env;
    out->lens = p.lens; out->sph = p.sph; out->tex = p.tex;
    out->shade = p.shade; out->fuse = p.fuse();
    out->full_state = p.full_state(); out->resolves_sky = p.resolves_sky(); out->instrumented = p.instrumented();
    static const uint32_t probe_iterations[3] = { 0u, 2u, 3u };
    for (int b = 0; b < 2; ++b) { out->single_loop[b] = p.single_loop(b != 0); out->generate_mode[b] = p.generate_mode(b != 0); }
    for (uint32_t choice = 0; choice < 4; ++choice)
        for (int i = 0; i < 3; ++i) out->kernel_for[choice][i] = p.kernel_for(choice, probe_iterations[i]);
}

void tp_decode(uint32_t flags, uint32_t tuned_kernel, int has_env, int has_specular, int has_lens, int has_sphere_light, int has_textures, tp_pipeline *out)
{
    fill(decode_pipeline(flags, tuned_kernel, has_env != 0, has_specular != 0, has_lens != 0, has_sphere_light != 0, has_textures != 0), out);
}

void tp_decode_default(uint32_t flags, uint32_t tuned_kernel, int has_env, int has_specular, int has_lens, int has_sphere_light, tp_pipeline *out)
{
    fill(decode_pipeline(flags, tuned_kernel, has_env != 0, has_specular != 0, has_lens != 0, has_sphere_light != 0), out);
}

int tp_extend_instantiated(int kernel, int fuse, int count, int nee, int env, int lens, int sph, int tex)
{
    return extend_instantiated(kernel, fuse, count != 0, nee != 0, env != 0, lens != 0, sph != 0, tex != 0);
}

}
