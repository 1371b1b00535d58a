// api.cpp — C ABI of libptrt.so (include/ptrt.h): ABI version and errors, context life cycle and tuning, tile layout, the read-backs and
// device pointers of a frame, pt_assemble_tiles. (pt_render: frame.cpp; ray queries: query.cpp; denoising: denoise_host.cpp; display: display_host.cpp; scenes: scene.cpp.)
// Stands where Renderer.CreateResources / CreateComputePipeline stand in the reference (RayTracing/Graphics/Renderer.cs:105-196, 293-403).
// HIP only: there is no CPU fallback anywhere in this library.
#include "context.h"
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>

using namespace ptrt;

namespace {
thread_local std::string g_err;
}

namespace ptrt {
pt_status layout_of(const pt_render_params *p, pt_tile_layout *o)
{
    if (!p || !o) return PT_ERR_INVALID_ARGUMENT;
    if (p->width == 0 || p->height == 0 || p->width > 32768 || p->height > 32768) return PT_ERR_INVALID_ARGUMENT;
    if (p->tile_size != 0 && p->tile_size != kTile) return PT_ERR_UNSUPPORTED;
    const uint32_t nr = p->nranks ? p->nranks : 1u;
    if (p->rank >= nr) return PT_ERR_INVALID_ARGUMENT;
    o->tile_size = kTile;
    o->tiles_x = (p->width + kTile - 1) / kTile;
    o->tiles_y = (p->height + kTile - 1) / kTile;
    o->n_tiles = o->tiles_x * o->tiles_y;
    o->tiles_mine = (o->n_tiles > p->rank) ? (o->n_tiles - p->rank + nr - 1) / nr : 0u;
    o->tiles_per_rank = (o->n_tiles + nr - 1) / nr;
    o->floats_per_tile = (uint64_t)kTilePixels * 4u;
    return PT_OK;
}
int context_device(const pt_context *c) { return c->device; }
hipStream_t context_stream(const pt_context *c) { return c->stream; }
void context_set_error(pt_context *c, const char *msg) { g_err = msg; if (c) c->err = msg; }
pt_status fail(pt_context *ctx, pt_status code, const char *fmt, ...)
{
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    context_set_error(ctx, buf);
    return code;
}
void context_drain(pt_context *c)
{
    for (auto &gs : c->group_stream) if (gs) (void)hipStreamSynchronize(gs);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
}
pt_status check_device_array(pt_context *c, const void *p, uint64_t bytes, const char *what, const char *who, const char *host_flag)
{
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess || (at.type != hipMemoryTypeDevice && !at.isManaged) || at.device != c->device) {
        (void)hipGetLastError();
        return fail(c, PT_ERR_INVALID_ARGUMENT, "%s: %s is not device memory of the context's device %d (host arrays: %s)", who, what, c->device, host_flag);
    }
    hipDeviceptr_t base = nullptr; size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) { (void)hipGetLastError(); return PT_OK; } // (range unknown: trust the caller)
    if ((const char *)p + bytes > (const char *)base + size)
        return fail(c, PT_ERR_INVALID_ARGUMENT, "%s: %s holds %llu bytes from the pointer on, the call needs %llu", who, what,
                    (unsigned long long)((const char *)base + size - (const char *)p), (unsigned long long)bytes);
    return PT_OK;
}
pt_status copy_out(pt_context *c, void *dst, const void *src, uint64_t need, size_t elem, uint64_t have, const char *unit)
{
    if (have < need) return fail(c, PT_ERR_INVALID_ARGUMENT, "buffer too small: need %llu %s", (unsigned long long)need, unit);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(dst, src, need * elem, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PT_OK;
}
} // namespace ptrt

extern "C" {

uint32_t pt_abi_version(void) { return PTRT_ABI_VERSION; }

const char *pt_last_error(const pt_context *ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

pt_status pt_context_create(const pt_device_desc *desc, pt_context **out)
{
    if (!out) return fail(nullptr, PT_ERR_INVALID_ARGUMENT, "pt_context_create: out is NULL");
    *out = nullptr;
    const int dev = desc ? desc->device_ordinal : 0;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, PT_ERR_NO_DEVICE, "no HIP device visible (%s); libptrt has no CPU backend",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (dev < 0 || dev >= ndev) return fail(nullptr, PT_ERR_INVALID_ARGUMENT, "device ordinal %d out of range [0,%d)", dev, ndev);
    hipDeviceProp_t prop;
    HIP_TRY(nullptr, hipGetDeviceProperties(&prop, dev));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, PT_ERR_NO_DEVICE, "device %d is %s; libptrt ships gfx950 (MI355X) code objects only", dev, prop.gcnArchName);
    HIP_TRY(nullptr, hipSetDevice(dev));
    pt_context *c = new (std::nothrow) pt_context();
    if (!c) return fail(nullptr, PT_ERR_OUT_OF_MEMORY, "host allocation failed");
    c->device = dev;
    if (desc && desc->stream) c->stream.borrow((hipStream_t)desc->stream);
    else if ((e = c->stream.create()) != hipSuccess) { delete c; return fail(nullptr, PT_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e)); } // (the text this failure has always had)
    bool ok = c->sizes.alloc() == hipSuccess;
    // host-mapped ring for the kernels' own size reports; a platform without mapped pinned memory falls back to a copy per launch
    if (ok && !c->sizes.can_map()) c->tuning.readback = 1u;
    for (uint32_t g = 0; ok && g < kMaxGroups; ++g) ok = c->group_stream[g].create() == hipSuccess && c->ev_join[g].create(false) == hipSuccess;
    ok = ok && c->ev_fork.create(false) == hipSuccess && c->ev_start.create() == hipSuccess && c->ev_stop.create() == hipSuccess;
    ok = ok && c->sizes.create_events() == hipSuccess;
    for (auto &ev : c->ev_probe) ok = ok && ev.create() == hipSuccess;
    for (auto &ev : c->query.ev) ok = ok && ev.create() == hipSuccess;
    ok = ok && c->counters.ensure(kCntTotalWords) == hipSuccess;
    if (!ok) { delete c; return fail(nullptr, PT_ERR_HIP, "context resource creation failed"); } // nothing runs yet: the owners give back what was made
    *out = c;
    return PT_OK;
}

pt_status pt_context_get_tuning(const pt_context *c, pt_tuning *o)
{
    if (!c || !o) return fail(nullptr, PT_ERR_INVALID_ARGUMENT, "pt_context_get_tuning: NULL argument");
    *o = c->tuning;
    return PT_OK;
}

pt_status pt_context_set_tuning(pt_context *c, const pt_tuning *t)
{
    if (!c || !t) return fail(c, PT_ERR_INVALID_ARGUMENT, "pt_context_set_tuning: NULL argument");
    if (t->bounces > 64) return fail(c, PT_ERR_INVALID_ARGUMENT, "tuning: bounces must be 0 (default) or 1..64");
    if (t->loops != 0 && t->loops != 1 && t->loops != 2 && t->loops != 4) return fail(c, PT_ERR_INVALID_ARGUMENT, "tuning: loops must be 0 (default), 1, 2 or 4");
    if (t->packed_chunk != 0 && (t->packed_chunk < 64 || t->packed_chunk > (1u << 20))) return fail(c, PT_ERR_INVALID_ARGUMENT, "tuning: packed_chunk must be 0 (default) or 64..2^20");
    if (t->lag != 0 && (t->lag < 2 || t->lag > kLag)) return fail(c, PT_ERR_INVALID_ARGUMENT, "tuning: lag must be 0 (default) or 2..%u", kLag);
    if (!(t->compact_below >= 0.f && t->compact_below <= 2.f) || !(t->sparse_below >= 0.f && t->sparse_below <= 1.f))
        return fail(c, PT_ERR_INVALID_ARGUMENT, "tuning: compact_below must be in [0,2], sparse_below in [0,1]");
    if (t->extend_kernel > kExtendKernelLast) return fail(c, PT_ERR_INVALID_ARGUMENT, "tuning: extend_kernel must be 0 (probed), 1 (one ray per lane), 2 (lane-packing) or 3 (pooled)");
    if (t->readback > 1) return fail(c, PT_ERR_INVALID_ARGUMENT, "tuning: readback must be 0 (mapped store) or 1 (copy per launch)");
    if (t->readback == 0 && !c->sizes.can_map()) return fail(c, PT_ERR_UNSUPPORTED, "tuning: readback 0 needs host-mapped pinned memory, which this platform did not provide");
    c->tuning = *t; // all or nothing: a refused call changes no field
    return PT_OK;
}

void pt_context_destroy(pt_context *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    context_drain(c); // nothing may still run on what the members give back
    delete c;
}

pt_status pt_tile_layout_query(const pt_render_params *p, pt_tile_layout *o)
{
    pt_status st = layout_of(p, o);
    if (st != PT_OK) return fail(nullptr, st, "invalid render params for tile layout");
    return PT_OK;
}

pt_status pt_framebuffer_read(pt_context *c, float *rgba, uint64_t n_floats)
{
    if (!c || !rgba) return fail(c, PT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!c->out.readable()) return fail(c, PT_ERR_NOT_COMMITTED, "no assembled frame (render with nranks == 1 or call pt_assemble_tiles)");
    return copy_out(c, rgba, c->out.fb.p, c->out.pixels() * 4, sizeof(float), n_floats, "floats");
}

pt_status pt_framebuffer_read_rgba8(pt_context *c, uint8_t *rgba8, uint64_t n_bytes)
{
    if (!c || !rgba8) return fail(c, PT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!c->out.readable()) return fail(c, PT_ERR_NOT_COMMITTED, "no assembled frame");
    return copy_out(c, rgba8, c->out.fb8.p, c->out.pixels() * 4, 1, n_bytes, "bytes");
}

pt_status pt_framebuffer_read_srgb8(pt_context *c, uint8_t *rgba8, uint64_t n_bytes)
{
    // display transform of the reference (SwapChain.cs:157-158 B8G8R8A8Srgb target, nearest-sampled UNORM8 source): a function of
    // the 8-bit value, so it is a 256-entry table over the UNORM8 read-back; alpha is linear in sRGB formats
    pt_status st = pt_framebuffer_read_rgba8(c, rgba8, n_bytes);
    if (st != PT_OK) return st;
    uint8_t lut[256];
    for (int q = 0; q < 256; ++q) {
        const double l = q / 255.0, e = l <= 0.0031308 ? 12.92 * l : 1.055 * std::pow(l, 1.0 / 2.4) - 0.055;
        lut[q] = (uint8_t)std::floor(255.0 * e + 0.5);
    }
    const uint64_t n = c->out.pixels() * 4;
    for (uint64_t i = 0; i < n; ++i) if ((i & 3u) != 3u) rgba8[i] = lut[rgba8[i]];
    return PT_OK;
}

pt_status pt_framebuffer_device_ptr(pt_context *c, void **dptr, uint64_t *n_floats)
{
    if (!c || !dptr) return fail(c, PT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!c->out.readable()) return fail(c, PT_ERR_NOT_COMMITTED, "no assembled frame");
    *dptr = c->out.fb.p;
    if (n_floats) *n_floats = c->out.pixels() * 4;
    return PT_OK;
}

pt_status pt_tiles_device_ptr(pt_context *c, void **dptr, uint64_t *n_floats)
{
    if (!c || !dptr) return fail(c, PT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!c->out.tile_slots()) return fail(c, PT_ERR_NOT_COMMITTED, "no path-traced frame yet");
    *dptr = c->out.tiles.p;
    if (n_floats) *n_floats = (uint64_t)c->out.tile_slots() * 4;
    return PT_OK;
}

pt_status pt_assemble_tiles(pt_context *c, const pt_render_params *p, const void *gathered, uint64_t n_floats)
{
    if (!c || !p || !gathered) return fail(c, PT_ERR_INVALID_ARGUMENT, "NULL argument");
    pt_tile_layout lay;
    pt_status st = layout_of(p, &lay);
    if (st != PT_OK) return fail(c, st, "pt_assemble_tiles: bad params");
    if (p->spp == 0) return fail(c, PT_ERR_INVALID_ARGUMENT, "spp == 0");
    const uint32_t nranks = p->nranks ? p->nranks : 1u;
    const uint64_t per_rank = (uint64_t)lay.tiles_per_rank * kTilePixels;
    if (n_floats < per_rank * nranks * 4) return fail(c, PT_ERR_INVALID_ARGUMENT, "gathered buffer too small: need %llu floats", (unsigned long long)(per_rank * nranks * 4));
    HIP_TRY(c, hipSetDevice(c->device));
    c->out.replace();
    HIP_TRY(c, c->out.resize(p->width, p->height));
    HIP_TRY(c, launch_assemble(c->stream, (const float4 *)gathered, nranks, (uint32_t)per_rank, p->width, p->height, lay.tiles_x, lay.n_tiles,
                               1.0f / (float)(((p->flags & PT_FLAG_ACCUMULATE) ? (uint64_t)p->sample_offset : 0u) + p->spp), c->out.fb.p, c->out.fb8.p));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->out.complete(FrameOutputs::Holds::path_traced);
    return PT_OK;
}

} // extern "C"
