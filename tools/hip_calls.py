"""Developer aid for comparing two builds call by call: one public call sequence and nothing else in the process. Run it under
`rocprofv3 --hip-trace --stats -- python3 tools/hip_calls.py <frame|nee|query>` once per build (PTRT_LIB picks the library) and compare
the calls per HIP API name. The extend kernel is forced, so that no timing decides what is launched.
frame: the headline scene (1M-triangle Cornell box, 1080p, 8 streams) at 8 spp; nee: the same with PT_FLAG_NEXT_EVENT;
query: one TraceRays of 2^16 rays and one Denoise of a 320 x 200 frame of the Cornell box with spheres."""
import sys; sys.path.insert(0, ".")
import numpy as np
import pathtracing_amd as P
N = P.native
what = sys.argv[1]
W, H = (320, 200) if what == "query" else (1920, 1080)
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
else:
    r.SetScene(P.make_scene(N.PT_SCENE_CORNELL_TESS, 1 << 20, 0x5EED0001, W, H), 0)
    r.Params = P.make_params(W, H, spp=8, max_depth=8, streams=8, flags=N.PT_FLAG_NEXT_EVENT if what == "nee" else 0)
    st = r.Render(0.0)
    print(f"{what}: {st.rays} rays, {st.iterations} launches, checksum {float(r.ReadFramebuffer().sum()):.6f}", flush=True)
r.Dispose()
