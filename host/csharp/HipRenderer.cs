// Compute-path replacement for RayTracing.Graphics.Renderer (Renderer.cs): same public shape
// (ctor / Init / Update / Render(delta) / Dispose), the Vulkan objects replaced by two opaque libptrt handles.
// NOT compiled here (no dotnet in the image) — see INTEGRATION.md.
using System;

namespace RayTracing.Graphics;

public unsafe class HipRenderer : IDisposable
{
    private bool _disposed;
    private void* _ctx, _scene;
    public PtRenderParams Params;
    public PtStats LastStats;
    public readonly uint Width, Height;

    public HipRenderer(uint width = 1920, uint height = 1080) // App.cs:27 window size
    {
        Width = width; Height = height;
        Params = new PtRenderParams { width = width, height = height, spp = 1, max_depth = 8, rr_start = 3, seed = 0x5EED0001,
                                      mode = (uint)PtMode.ReferenceSphere, ray_eps = 1e-4f, nranks = 1, streams = 8 };
    }

    // Renderer.Init (Renderer.cs:66-84): device + resources + compute pipeline
    public void Init(int device = 0)
    {
        if (Ptrt.pt_abi_version() != Ptrt.AbiVersion) throw new Exception($"libptrt has ABI version {Ptrt.pt_abi_version()}, this binding expects {Ptrt.AbiVersion}");
        PtDeviceDesc d = new() { device_ordinal = device };
        void* c; Ptrt.Check(Ptrt.pt_context_create(&d, &c)); _ctx = c;
    }

    public void LoadSyntheticScene(PtSceneKind kind, uint detail = 0, uint seed = 0x5EED0001, uint bvhWidth = 0)
    {
        PtSceneCounts n; PtCamera cam; float* sky = stackalloc float[3];
        Ptrt.Check(Ptrt.pt_scenegen((uint)kind, detail, seed, Width, Height, &n, null, null, null, null, null, null, null));
        float[] verts = new float[n.n_tris * 9]; uint[] tmat = new uint[n.n_tris];
        float[] sph = new float[Math.Max(1, n.n_spheres * 4)]; uint[] smat = new uint[Math.Max(1, n.n_spheres)];
        PtMaterial[] mats = new PtMaterial[n.n_mats];
        fixed (float* v = verts, s = sph) fixed (uint* tm = tmat, sm = smat) fixed (PtMaterial* m = mats)
        {
            Ptrt.Check(Ptrt.pt_scenegen((uint)kind, detail, seed, Width, Height, &n, v, tm, s, sm, m, &cam, sky));
            if (_scene != null) Ptrt.pt_scene_destroy(_scene);
            void* sc; Ptrt.Check(Ptrt.pt_scene_create(_ctx, &sc), _ctx); _scene = sc;
            Ptrt.Check(Ptrt.pt_scene_set_triangles(sc, v, tm, n.n_tris), _ctx);
            Ptrt.Check(Ptrt.pt_scene_set_spheres(sc, s, sm, n.n_spheres), _ctx);
            Ptrt.Check(Ptrt.pt_scene_set_materials(sc, m, n.n_mats), _ctx);
            Ptrt.Check(Ptrt.pt_scene_set_camera(sc, &cam), _ctx);
            Ptrt.Check(Ptrt.pt_scene_set_sky(sc, sky), _ctx);
            Ptrt.Check(Ptrt.pt_scene_commit(sc, bvhWidth), _ctx);
        }
        Params.mode = (uint)PtMode.PathTrace;
    }

    public void Update(float deltaTime) { } // empty in the reference too (Renderer.cs:86-89)

    // Renderer.Render (Renderer.cs:933-1004) minus acquire/draw/present: ComputeFrame + fence wait
    public void Render(float delta) => ComputeFrame(delta);

    // Renderer.ComputeFrame (Renderer.cs:1006-1040); pt_render returns after the stream is idle (= WaitForFences, :972)
    private void ComputeFrame(float delta)
    {
        fixed (PtRenderParams* p = &Params) fixed (PtStats* st = &LastStats)
            Ptrt.Check(Ptrt.pt_render(_ctx, Params.mode == (uint)PtMode.PathTrace ? _scene : null, p, st), _ctx);
    }

    public float[] ReadFramebuffer()
    {
        float[] rgba = new float[(ulong)Width * Height * 4];
        fixed (float* p = rgba) Ptrt.Check(Ptrt.pt_framebuffer_read(_ctx, p, (ulong)rgba.Length), _ctx);
        return rgba;
    }

    public byte[] ReadFramebufferRgba8() // the R8G8B8A8Unorm image of Renderer.cs:124
    {
        byte[] px = new byte[(ulong)Width * Height * 4];
        fixed (byte* p = px) Ptrt.Check(Ptrt.pt_framebuffer_read_rgba8(_ctx, p, (ulong)px.Length), _ctx);
        return px;
    }

    public byte[] ReadFramebufferSrgb8() // what the reference's B8G8R8A8Srgb swapchain shows of that image (SwapChain.cs:157-158)
    {
        byte[] px = new byte[(ulong)Width * Height * 4];
        fixed (byte* p = px) Ptrt.Check(Ptrt.pt_framebuffer_read_srgb8(_ctx, p, (ulong)px.Length), _ctx);
        return px;
    }

    // scheduling knobs (none changes a pixel): read, modify, write back
    public PtTuning Tuning
    {
        get { PtTuning t; Ptrt.Check(Ptrt.pt_context_get_tuning(_ctx, &t), _ctx); return t; }
        set { Ptrt.Check(Ptrt.pt_context_set_tuning(_ctx, &value), _ctx); }
    }

    // Hemisphere gathers on the current scene (docs/SPEC.md §12): ambient occlusion, sky irradiance and the bent normal of a bake. points: 8
    // floats per point {p.xyz, 0, n.xyz, 0}; returns 8 floats per point {E.rgb, visibility, bent.xyz, 0} (visibility -1: an invalid point).
    // samples cosine-weighted occlusion rays per point are made, traced and summed on the device. Host arrays: the library stages them.
    public float[] Gather(float[] points, uint samples = 64, uint seed = 0, float maxDistance = 0f, float rayEps = 1e-3f,
                          uint sampleOffset = 0, uint pointOffset = 0)
    {
        if (points.Length % 8 != 0) throw new ArgumentException("points: 8 floats per point");
        var rows = new float[points.Length];
        var gp = new PtGatherParams { samples = samples, seed = seed, sample_offset = sampleOffset, point_offset = pointOffset,
                                      max_distance = maxDistance, ray_eps = rayEps, flags = (uint)PtGatherFlags.HostMemory };
        PtStats st;
        fixed (float* p = points) fixed (float* o = rows)
            Ptrt.Check(Ptrt.pt_gather(_ctx, _scene, p, o, (ulong)(points.Length / 8), &gp, &st), _ctx);
        return rows;
    }

    // Path-traced gathers (docs/SPEC.md §12.1): Gather's points and rows, with every sample a whole path of at most maxDepth segments that
    // starts at the point (Russian roulette from depth rrStart on). E carries emissive surfaces and bounced light; visibility and bent are Gather's.
    // nextEvent (§12.2): light samples with MIS at the point and at the paths' Lambert vertices; with maxDepth 1 a direct-light bake.
    // sphereLights (§7.1; needs nextEvent): the scene's emissive spheres are lights too, sampled by the cone they subtend.
    public float[] GatherPaths(float[] points, uint samples = 64, uint seed = 0, float maxDistance = 0f, float rayEps = 1e-3f,
                               uint sampleOffset = 0, uint pointOffset = 0, uint maxDepth = 8, uint rrStart = 3, bool nextEvent = false,
                               bool sphereLights = false)
    {
        if (points.Length % 8 != 0) throw new ArgumentException("points: 8 floats per point");
        var rows = new float[points.Length];
        var gp = new PtGatherParams { samples = samples, seed = seed, sample_offset = sampleOffset, point_offset = pointOffset,
                                      max_distance = maxDistance, ray_eps = rayEps, flags = (uint)PtGatherFlags.HostMemory };
        var pp = new PtGatherPathParams { max_depth = maxDepth, rr_start = rrStart, flags = (nextEvent ? (uint)PtGatherPathFlags.NextEvent : 0) | (sphereLights ? (uint)PtGatherPathLights.SphereLights : 0) };
        PtStats st;
        fixed (float* p = points) fixed (float* o = rows)
            Ptrt.Check(Ptrt.pt_gather_paths(_ctx, _scene, p, o, (ulong)(points.Length / 8), &gp, &pp, &st), _ctx);
        return rows;
    }

    // Ray queries on the current scene (docs/SPEC.md §4.2). rays: 8 floats per ray {o.xyz, tmax, d.xyz, 0} (|d| = 1 for spheres);
    // returns 4 floats per ray {t, prim id bits, u, v}, a miss = {+inf, 0xFFFFFFFF bits, 0, 0}. Host arrays: the library stages them.
    public float[] TraceRays(float[] rays, bool occlusion = false)
    {
        if (rays.Length % 8 != 0) throw new ArgumentException("rays: 8 floats per ray");
        var hits = new float[rays.Length / 2];
        uint flags = (uint)PtTraceFlags.HostMemory | (occlusion ? (uint)PtTraceFlags.Occlusion : 0u);
        PtStats st;
        fixed (float* r = rays) fixed (float* h = hits)
            Ptrt.Check(Ptrt.pt_trace_rays(_ctx, _scene, r, h, (ulong)(rays.Length / 8), flags, &st), _ctx);
        return hits;
    }

    // Move the current scene's geometry without a new commit (docs/SPEC.md §4.3), e.g. from an application's Update(deltaTime):
    // verts = 9 floats per triangle (the committed count and order), spheres = 4 floats per sphere {centre, radius}; either may be null.
    // The tree keeps its topology, the picture is exactly a fresh commit's; pt_bvh_info.sah_cost says when a new commit would pay again.
    // Returns the triangle update's stats (gpu_ms).
    public PtStats UpdateGeometry(float[] verts, float[] spheres = null)
    {
        PtStats st = default;
        if (verts != null)
        {
            if (verts.Length % 9 != 0) throw new ArgumentException("verts: 9 floats per triangle");
            fixed (float* v = verts)
                Ptrt.Check(Ptrt.pt_scene_update_triangles(_scene, v, (ulong)(verts.Length / 9), (uint)PtUpdateFlags.HostMemory, &st), _ctx);
        }
        if (spheres != null)
        {
            if (spheres.Length % 4 != 0) throw new ArgumentException("spheres: 4 floats per sphere");
            fixed (float* p = spheres) Ptrt.Check(Ptrt.pt_scene_update_spheres(_scene, p, (ulong)(spheres.Length / 4)), _ctx);
        }
        return st;
    }

    // Denoise the last frame (docs/SPEC.md §8): first-hit guides traced on the current scene, then the edge-aware à-trous filter.
    // Zeros mean the defaults. The framebuffer and the accumulated sums stay as they are; ReadDenoised / ReadGuides hold until the
    // next Render. Returns the stats (extend_ms = guide pass, other_ms = filter passes).
    public PtStats Denoise(uint iterations = 0, float sigmaColor = 0f, float sigmaNormal = 0f, float sigmaDepth = 0f, float sigmaAlbedo = 0f,
                           bool guidesOnly = false, bool edgeStops = true)
    {
        var dp = new PtDenoiseParams { iterations = iterations, sigma_color = sigmaColor, sigma_normal = sigmaNormal, sigma_depth = sigmaDepth,
                                       sigma_albedo = sigmaAlbedo,
                                       flags = (guidesOnly ? (uint)PtDenoiseFlags.GuidesOnly : 0u) | (edgeStops ? 0u : (uint)PtDenoiseFlags.NoEdgeStops) };
        PtStats st;
        Ptrt.Check(Ptrt.pt_denoise(_ctx, _scene, &dp, &st), _ctx);
        return st;
    }

    public float[] ReadDenoised()
    {
        float[] rgba = new float[(ulong)Width * Height * 4];
        fixed (float* p = rgba) Ptrt.Check(Ptrt.pt_denoised_read(_ctx, p, (ulong)rgba.Length), _ctx);
        return rgba;
    }

    // 8 floats per pixel: front-facing normal, t, albedo, prim id bits (a miss: t = +inf, id 0xFFFFFFFF) — a host denoiser's features
    public float[] ReadGuides()
    {
        float[] g = new float[(ulong)Width * Height * 8];
        fixed (float* p = g) Ptrt.Check(Ptrt.pt_guides_read(_ctx, p, (ulong)g.Length), _ctx);
        return g;
    }

    // Move the current scene's camera (no new commit needed)
    public void SetCamera(PtCamera cam) { Ptrt.Check(Ptrt.pt_scene_set_camera(_scene, &cam), _ctx); }

    // Give the current scene an environment map (docs/SPEC.md §11): n x n texels of linear RGB in octahedral layout, or null to remove
    // it. No new commit needed; while set it replaces the sky on every miss, and NextEvent frames sample it as a light.
    public void SetEnvironment(float[] rgb, uint n)
    {
        if (rgb == null) { Ptrt.Check(Ptrt.pt_scene_set_environment(_scene, null, 0), _ctx); return; }
        if ((ulong)rgb.Length < (ulong)n * n * 3) throw new ArgumentException("SetEnvironment: fewer than n * n * 3 floats");
        fixed (float* p = rgb) Ptrt.Check(Ptrt.pt_scene_set_environment(_scene, p, n), _ctx);
    }

    // Give the current scene a thin lens (docs/SPEC.md §3.1: depth of field): an aperture of `radius` world units focused at
    // `focusDistance`; radius 0 is the pinhole, and ClearLens removes the lens. No new commit needed; restart accumulation after a change.
    public void SetLens(float radius, float focusDistance)
    {
        var lens = new PtLens { radius = radius, focus_distance = focusDistance };
        Ptrt.Check(Ptrt.pt_scene_set_lens(_scene, &lens), _ctx);
    }
    public void ClearLens() { Ptrt.Check(Ptrt.pt_scene_set_lens(_scene, null), _ctx); }

    // Albedo textures (docs/SPEC.md §13): per-triangle UVs (six floats per triangle, null removes them), texture `index` (width x height
    // texels of linear RGB, null removes it; flags 1 = nearest texel) and one texture index or 0xFFFFFFFF per material (null removes the
    // binding). All three take effect with the next Commit. Not there: textured spheres, emission or roughness maps, mip-mapping,
    // textures under a lens or with sphere lights, textured path gathers.
    public void SetTriangleUvs(float[] uv6)
    {
        if (uv6 == null) { Ptrt.Check(Ptrt.pt_scene_set_triangle_uvs(_scene, null, 0), _ctx); return; }
        fixed (float* p = uv6) Ptrt.Check(Ptrt.pt_scene_set_triangle_uvs(_scene, p, (ulong)uv6.Length / 6), _ctx);
    }
    public void SetTexture(uint index, float[] rgb, uint width, uint height, uint flags = 0)
    {
        if (rgb == null) { Ptrt.Check(Ptrt.pt_scene_set_texture(_scene, index, null, 0, 0, 0), _ctx); return; }
        if ((ulong)rgb.Length < (ulong)width * height * 3) throw new ArgumentException("SetTexture: fewer than width * height * 3 floats");
        fixed (float* p = rgb) Ptrt.Check(Ptrt.pt_scene_set_texture(_scene, index, p, width, height, flags), _ctx);
    }
    public void SetMaterialTextures(uint[] textureOfMaterial)
    {
        if (textureOfMaterial == null) { Ptrt.Check(Ptrt.pt_scene_set_material_textures(_scene, null, 0), _ctx); return; }
        fixed (uint* p = textureOfMaterial) Ptrt.Check(Ptrt.pt_scene_set_material_textures(_scene, p, (ulong)textureOfMaterial.Length), _ctx);
    }
    public PtTextureInfo TextureInfo(uint index) { PtTextureInfo i; Ptrt.Check(Ptrt.pt_scene_texture_info(_scene, index, &i), _ctx); return i; }
    public void Commit(uint bvhWidth = 0) { Ptrt.Check(Ptrt.pt_scene_commit(_scene, bvhWidth), _ctx); }

    // Temporal accumulation (docs/SPEC.md §9), the call of a render-every-frame loop whose camera or geometry moves: reprojects the
    // previous call's accumulated image to this frame, blends the last Render in, and (filter = true) runs Denoise's filter over the
    // result. Zeros mean the defaults. ReadTemporal / ReadHistoryLength / ReadDenoised hold until the next Render; the history itself
    // is kept by the context until reset = true or a change of size. Returns the stats (paths = pixels that took history,
    // shade_ms = the temporal pass). motion = true (PT_TEMPORAL_MOTION, §9.1) also records the geometry the call was traced on, and
    // pixels of primitives that UpdateGeometry moved since the previous such call take their history from where their surface point was.
    public PtStats DenoiseTemporal(uint maxHistory = 0, float planeTolerance = 0f, float normalMin = 0f, bool reset = false, bool matchIds = false,
                                   bool filter = true, uint iterations = 0, bool motion = false)
    {
        var tp = new PtTemporalParams { max_history = maxHistory, plane_tolerance = planeTolerance, normal_min = normalMin,
                                        flags = (reset ? (uint)PtTemporalFlags.Reset : 0u) | (matchIds ? (uint)PtTemporalFlags.MatchIds : 0u)
                                                | (motion ? (uint)PtTemporalFlags.Motion : 0u) };
        var dp = new PtDenoiseParams { iterations = iterations };
        PtStats st;
        Ptrt.Check(Ptrt.pt_denoise_temporal(_ctx, _scene, &tp, filter ? &dp : null, &st), _ctx);
        return st;
    }

    public float[] ReadTemporal()
    {
        float[] rgba = new float[(ulong)Width * Height * 4];
        fixed (float* p = rgba) Ptrt.Check(Ptrt.pt_temporal_read(_ctx, p, (ulong)rgba.Length), _ctx);
        return rgba;
    }

    // one float per pixel: how many frames the pixel's accumulated colour stands for (1 = it took no history)
    public float[] ReadHistoryLength()
    {
        float[] len = new float[(ulong)Width * Height];
        fixed (float* p = len) Ptrt.Check(Ptrt.pt_temporal_history_read(_ctx, p, (ulong)len.Length), _ctx);
        return len;
    }

    // The display stage (docs/SPEC.md §10), what stands where the reference's display pass samples the image (Renderer.cs:1042-1121):
    // the frame, the denoised or the accumulated image times an exposure, through a tone curve, encoded to sRGB8 (linear: UNORM8) on
    // the device. autoExposure meters the exposure from a luminance histogram and adapts it from call to call (adapt, key, trims per
    // mille); exposure then compensates on top. Zeros mean the defaults. ReadDisplay / DisplayInfo / ReadDisplayHistogram hold until
    // the next Render; the adapted exposure is kept by the context until reset = true.
    public PtStats Display(PtDisplaySource source = PtDisplaySource.Frame, PtToneCurve curve = PtToneCurve.Clamp, float exposure = 0f,
                           bool autoExposure = false, float white = 0f, float key = 0f, float adapt = 0f, uint trimLow = 0, uint trimHigh = 0,
                           bool linear = false, bool reset = false)
    {
        var dp = new PtDisplayParams { source = (uint)source, curve = (uint)curve, exposure = exposure, white = white, key = key, adapt = adapt,
                                       trim_low = trimLow, trim_high = trimHigh,
                                       flags = (autoExposure ? (uint)PtDisplayFlags.AutoExposure : 0u) | (linear ? (uint)PtDisplayFlags.Linear : 0u)
                                             | (reset ? (uint)PtDisplayFlags.ResetAdaptation : 0u) };
        PtStats st;
        Ptrt.Check(Ptrt.pt_display(_ctx, &dp, &st), _ctx);
        return st;
    }

    public byte[] ReadDisplay()
    {
        byte[] rgba = new byte[(ulong)Width * Height * 4];
        fixed (byte* p = rgba) Ptrt.Check(Ptrt.pt_display_read(_ctx, p, (ulong)rgba.Length), _ctx);
        return rgba;
    }

    public PtDisplayInfo DisplayInfo()
    {
        PtDisplayInfo info;
        Ptrt.Check(Ptrt.pt_display_info_read(_ctx, &info), _ctx);
        return info;
    }

    public uint[] ReadDisplayHistogram()
    {
        uint[] bins = new uint[512];
        fixed (uint* p = bins) Ptrt.Check(Ptrt.pt_display_histogram_read(_ctx, p, (ulong)bins.Length), _ctx);
        return bins;
    }

    internal void* Context => _ctx;
    internal void* Scene => _scene;

    protected virtual void Dispose(bool disposing)
    {
        if (_disposed) return;
        if (_scene != null) Ptrt.pt_scene_destroy(_scene);
        if (_ctx != null) Ptrt.pt_context_destroy(_ctx);
        _scene = null; _ctx = null; _disposed = true;
    }
    public void Dispose() { Dispose(true); GC.SuppressFinalize(this); }
    ~HipRenderer() { Dispose(false); }
}

// One frame over several GPUs of the node (include/ptrt.h pt_comm): a HipRenderer per device, the same scene on each, tiles dealt
// round-robin, one ncclGather per frame inside libptrt. The reference is single-device (GraphicsDevice.cs:176-183); this is what stands
// above its Renderer when the node has 8 GPUs. NOT compiled here (no dotnet in the image).
public unsafe class HipMultiRenderer : IDisposable
{
    private readonly HipRenderer[] _r;
    private void* _comm;
    public PtRenderParams Params;
    public PtStats[] LastStats;

    private readonly uint _commFlags;

    // oneDevice: every rank gets its own context on device 0 and the tiles are exchanged by device copies (PtCommFlags.CopyExchange)
    public HipMultiRenderer(int gpus, uint width = 1920, uint height = 1080, bool oneDevice = false)
    {
        _commFlags = oneDevice ? (uint)PtCommFlags.CopyExchange : 0u;
        _r = new HipRenderer[gpus];
        for (int i = 0; i < gpus; i++) { _r[i] = new HipRenderer(width, height); _r[i].Init(oneDevice ? 0 : i); }
        Params = _r[0].Params;
        LastStats = new PtStats[gpus];
    }

    public void LoadSyntheticScene(PtSceneKind kind, uint detail = 0)
    {
        foreach (HipRenderer r in _r) r.LoadSyntheticScene(kind, detail); // replicated scene
        Params.mode = (uint)PtMode.PathTrace;
        void** ctxs = stackalloc void*[_r.Length];
        for (int i = 0; i < _r.Length; i++) ctxs[i] = _r[i].Context;
        if (_comm != null) Ptrt.pt_comm_destroy(_comm);
        void* c; Ptrt.Check(Ptrt.pt_comm_create(ctxs, (uint)_r.Length, 0, _commFlags, &c)); _comm = c;
    }

    public void Render(float delta)
    {
        void** scenes = stackalloc void*[_r.Length];
        for (int i = 0; i < _r.Length; i++) scenes[i] = _r[i].Scene;
        fixed (PtRenderParams* p = &Params) fixed (PtStats* st = LastStats)
            Ptrt.Check(Ptrt.pt_comm_render(_comm, scenes, p, st), _r[0].Context);
    }

    public HipRenderer Root => _r[0]; // holds the assembled frame

    public void Dispose()
    {
        if (_comm != null) Ptrt.pt_comm_destroy(_comm);
        _comm = null;
        foreach (HipRenderer r in _r) r.Dispose();
        GC.SuppressFinalize(this);
    }
}
