"""Developer aid for comparing two builds call by call: one public call sequence and nothing else in the process. Run it under
`rocprofv3 --hip-trace --stats -- python3 tools/hip_calls.py <frame|nee|query|post>` once per build (PTRT_LIB picks the library) and compare
the calls per HIP API name. The extend kernel is forced, so that no timing decides what is launched.
frame: the headline scene (1M-triangle Cornell box, 1080p, 8 streams) at 8 spp; nee: the same with PT_FLAG_NEXT_EVENT;
query: one TraceRays of 2^16 rays and one Denoise of a 320 x 200 frame of the Cornell box with spheres;
post: on that box at 320 x 200 and 2 spp, every post-process call: Render, Denoise, DenoiseTemporal(motion), the spheres moved, Render,
DenoiseTemporal(motion) (the motion kernel), the camera moved, Render, DenoiseTemporal, two metered Displays, then one of each read
call and device pointer with a checksum per read."""
import ctypes as C
import sys; sys.path.insert(0, ".")
import numpy as np
import pathtracing_amd as P
N = P.native
what = sys.argv[1]
W, H = (320, 200) if what in ("query", "post") else (1920, 1080)
r = P.Renderer(P.Window(W, H)); r.Init()
r.SetTuning(extend_kernel=1)
if what == "query":
    r.SetScene(P.make_scene(N.PT_SCENE_CORNELL_GLASS, 0, 0x5EED0001, W, H), 0)
    r.Params = P.make_params(W, H, spp=2, max_depth=8, streams=2)
    r.Render(0.0)
    rng = np.random.default_rng(1)
    d = rng.normal(size=(1 << 16, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    hits, st = r.TraceRays((np.zeros_like(d), d))
    dn = r.Denoise()
    print(f"query: {st.rays} rays, {int(np.isfinite(hits[:, 0]).sum())} hits; denoise {dn.rays} guide rays, {dn.iterations} passes, checksum {float(r.ReadDenoised().sum()):.6f}", flush=True)
elif what == "post":
    sd = P.make_scene(N.PT_SCENE_CORNELL_GLASS, 0, 0x5EED0001, W, H)
    r.SetScene(sd, 0)
    r.Params = P.make_params(W, H, spp=2, max_depth=8, streams=2)
    r.Render(0.0)
    dn = r.Denoise()
    t0 = r.DenoiseTemporal(motion=True)
    r.UpdateGeometry(spheres=np.asarray(sd.spheres, np.float32) + np.float32([0.0, 0.0625, 0.0, 0.0]))
    r.Render(0.0)
    t1 = r.DenoiseTemporal(motion=True)
    cam = N.pt_camera.from_buffer_copy(sd.cam)
    cam.origin[0] += 0.125
    r.SetCamera(cam)
    r.Render(0.0)
    t2 = r.DenoiseTemporal()
    d0 = r.Display(source="temporal", curve="aces", auto=True, adapt=0.5)
    d1 = r.Display(source="denoised", curve="aces", auto=True, adapt=0.5)
    print(f"post: denoise {dn.rays} guide rays, {dn.iterations} passes; temporal took {t0.paths} / {t1.paths} / {t2.paths}, moved "
          f"{t0.reserved[0]} / {t1.reserved[0]} / {t2.reserved[0]}; display {d0.paths} / {d1.paths} pixels", flush=True)
    info = r.DisplayInfo()
    reads = {"framebuffer": r.ReadFramebuffer(), "denoised": r.ReadDenoised(), "guides": np.nan_to_num(r.ReadGuides()[..., :7], posinf=0.0),
             "temporal": r.ReadTemporal(), "history": r.ReadHistoryLength(), "display": r.ReadDisplay(),
             "display_info": np.frombuffer(bytes(info), np.uint32), "display_histogram": r.ReadDisplayHistogram()}
    for name, a in reads.items():
        print(f"post: {name} checksum {float(a.astype(np.float64).sum()):.6f}", flush=True)
    for name in ("pt_framebuffer_device_ptr", "pt_denoised_device_ptr", "pt_temporal_device_ptr", "pt_display_device_ptr"):
        ptr, n = C.c_void_p(), C.c_uint64()
        status = getattr(N.lib, name)(r._ctx, C.byref(ptr), C.byref(n))
        print(f"post: {name} status {status}, {n.value} elements, {'set' if ptr.value else 'NULL'}", flush=True)
else:
    r.SetScene(P.make_scene(N.PT_SCENE_CORNELL_TESS, 1 << 20, 0x5EED0001, W, H), 0)
    r.Params = P.make_params(W, H, spp=8, max_depth=8, streams=8, flags=N.PT_FLAG_NEXT_EVENT if what == "nee" else 0)
    st = r.Render(0.0)
    print(f"{what}: {st.rays} rays, {st.iterations} launches, checksum {float(r.ReadFramebuffer().sum()):.6f}", flush=True)
r.Dispose()
