"""Host side above the C ABI, mirroring the reference's object shape
`Program -> App -> Renderer.{Init, Update, Render(dt)} -> ComputeFrame(dt)`
(RayTracing/Program.cs:1-9, App.cs:7-68, Graphics/Renderer.cs:59-89, 933-1004, 1006-1040).

The reference's host language is C# (no `dotnet` in this image — see INTEGRATION.md for the P/Invoke binding and
host/csharp for the C# sources); this Python mirror keeps the same names, argument meaning and error behaviour:
every failure raises (the reference does `throw new Exception(...)`, e.g. Renderer.cs:1022-1025), objects are
disposable, `Render(delta)` is synchronous like the compute-fence wait at Renderer.cs:970-972.
Everything here is plumbing around libptrt.so; no pixel is computed in Python.
"""
import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _native as N

MATERIAL_DTYPE = np.dtype([("kind", "<u4"), ("albedo", "<f4", 3), ("emission", "<f4", 3), ("roughness", "<f4"),
                           ("ior", "<f4"), ("pad", "<u4", 3)])
assert MATERIAL_DTYPE.itemsize == 48


class PtException(Exception):
    """Raised for every non-zero pt_status (the reference throws System.Exception on every Vulkan failure)."""

    def __init__(self, status, message):
        super().__init__(f"ptrt status {status}: {message}")
        self.status = status


def _check(status, ctx=None):
    if status != N.PT_OK:
        msg = N.lib.pt_last_error(ctx)
        raise PtException(status, msg.decode("utf-8", "replace") if msg else "")


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@dataclass
class SceneData:
    """Host-side scene arrays — what replaces the shader literals of Test.hlsl:6,8,12,13."""
    verts: np.ndarray = field(default_factory=lambda: np.zeros((0, 9), np.float32))
    tri_mat: np.ndarray = field(default_factory=lambda: np.zeros((0,), np.uint32))
    spheres: np.ndarray = field(default_factory=lambda: np.zeros((0, 4), np.float32))
    sph_mat: np.ndarray = field(default_factory=lambda: np.zeros((0,), np.uint32))
    mats: np.ndarray = field(default_factory=lambda: np.zeros((0,), MATERIAL_DTYPE))
    cam: N.pt_camera = field(default_factory=N.pt_camera)
    sky: np.ndarray = field(default_factory=lambda: np.zeros(3, np.float32))
    environment: np.ndarray = None  # optional n x n x 3 octahedral map (docs/SPEC.md §11); SetScene applies it
    # Albedo textures (docs/SPEC.md §13), all optional; SetScene passes them on before the commit
    uvs: np.ndarray = None                # (triangles, 6): (s, t) at v0, v1, v2
    textures: dict = None                 # index -> H x W x 3 linear RGB, or (H x W x 3, flags) with flags = native.PT_TEXTURE_NEAREST
    material_textures: np.ndarray = None  # (materials,): a texture index or native.PT_NO_TEXTURE


def _octahedral_directions(n, sub):
    """Unit directions (float64, (n, n, sub, sub, 3), indexed row, column, sub-row, sub-column) of a sub x sub grid of points in every
    texel of the n x n octahedral map: docs/SPEC.md §11's decode, in numpy."""
    t = (np.arange(n * sub) + 0.5) * (2.0 / (n * sub)) - 1.0
    u, v = np.meshgrid(t, t)  # v varies along rows
    z = 1.0 - np.abs(u) - np.abs(v)
    x = np.where(z < 0, (1.0 - np.abs(v)) * np.copysign(1.0, u), u)
    y = np.where(z < 0, (1.0 - np.abs(u)) * np.copysign(1.0, v), v)
    d = np.stack([x, y, z], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return d.reshape(n, sub, n, sub, 3).transpose(0, 2, 1, 3, 4)


def _octahedral_mean(values, n, sub):
    """Mean of per-point values (n, n, sub, sub, 3) over each texel's solid angle: the points weigh s^3 (d omega = s^3 dA, §11)."""
    d = _octahedral_directions(n, sub)
    w = (np.abs(d).sum(-1) ** 3)[..., None]
    return ((values * w).sum((2, 3)) / w.sum((2, 3))).astype(np.float32)


def environment_from_latlong(img, n, sub=4):
    """Resample a latitude-longitude image (rows from the +y pole down, columns by azimuth atan2(x, -z) from -pi to pi, 3 channels) to
    the n x n octahedral map pt_scene_set_environment takes: every texel is the solid-angle mean of a fixed sub x sub grid of nearest
    lookups. Host code: libm is allowed here, the device never sees a latitude or a longitude."""
    img = np.asarray(img, np.float64)
    h, w = img.shape[:2]
    d = _octahedral_directions(n, sub)
    row = np.clip((np.arccos(np.clip(d[..., 1], -1.0, 1.0)) / np.pi * h).astype(int), 0, h - 1)
    col = np.clip(((np.arctan2(d[..., 0], -d[..., 2]) / (2.0 * np.pi) + 0.5) * w).astype(int), 0, w - 1)
    return _octahedral_mean(img[row, col, :3], n, sub)


def sun_sky_environment(n, sun_dir, sun_rgb, sun_cos, sky_rgb, sub=4):
    """A deterministic n x n octahedral map: `sky_rgb` everywhere plus `sun_rgb` inside the cone of directions d with
    dot(d, sun_dir) >= sun_cos (a texel the cone's edge crosses gets the covered share of a fixed sub x sub grid)."""
    s = np.asarray(sun_dir, np.float64)
    s = s / np.linalg.norm(s)
    d = _octahedral_directions(n, sub)
    inside = ((d @ s) >= sun_cos)[..., None]
    return _octahedral_mean(np.asarray(sky_rgb, np.float64) + inside * np.asarray(sun_rgb, np.float64), n, sub)


def texture_from_srgb8(img):
    """An H x W x 3 (or 4: alpha dropped) uint8 sRGB image as the linear-RGB float32 texels pt_scene_set_texture takes: the sRGB
    electro-optical transfer function, decoded here on the host (the device never sees an encoded texel)."""
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (3, 4):
        raise ValueError(f"texture_from_srgb8 takes an H x W x 3 or 4 uint8 image, got {a.dtype} {a.shape}")
    c = a[..., :3].astype(np.float64) / 255.0
    lin = np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)
    return np.ascontiguousarray(lin, np.float32)


def make_scene(kind, detail=0, seed=0x5EED0001, width=1920, height=1080):
    """Deterministic synthetic scenes C1..C5 from the library's host-only generator."""
    cnt = N.pt_scene_counts()
    cam = N.pt_camera()
    _check(N.lib.pt_scenegen(kind, detail, seed, width, height, C.byref(cnt), None, None, None, None, None, None, None))
    s = SceneData(
        verts=np.zeros((cnt.n_tris, 9), np.float32), tri_mat=np.zeros(cnt.n_tris, np.uint32),
        spheres=np.zeros((cnt.n_spheres, 4), np.float32), sph_mat=np.zeros(cnt.n_spheres, np.uint32),
        mats=np.zeros(cnt.n_mats, MATERIAL_DTYPE), cam=cam, sky=np.zeros(3, np.float32))
    _check(N.lib.pt_scenegen(kind, detail, seed, width, height, C.byref(cnt), _ptr(s.verts), _ptr(s.tri_mat),
                             _ptr(s.spheres), _ptr(s.sph_mat), _ptr(s.mats), C.byref(cam), _ptr(s.sky)))
    return s


def build_bvh_detached(scene, bvh_width=0):
    """Run the library's host-side BVH builder on a detached (context-less) scene; returns (pt_bvh_info, nodes, tris48).
    No device is touched — this is how the builder is checked on machines without a GPU."""
    s = C.c_void_p()
    _check(N.lib.pt_scene_create(None, C.byref(s)))
    try:
        verts = np.ascontiguousarray(scene.verts, np.float32)
        tri_mat = np.ascontiguousarray(scene.tri_mat, np.uint32)
        spheres = np.ascontiguousarray(scene.spheres, np.float32)
        sph_mat = np.ascontiguousarray(scene.sph_mat, np.uint32)
        mats = np.ascontiguousarray(scene.mats)
        _check(N.lib.pt_scene_set_triangles(s, _ptr(verts), _ptr(tri_mat), len(tri_mat)))
        _check(N.lib.pt_scene_set_spheres(s, _ptr(spheres), _ptr(sph_mat), len(sph_mat)))
        _check(N.lib.pt_scene_set_materials(s, _ptr(mats), len(mats)))
        _check(N.lib.pt_scene_set_camera(s, C.byref(scene.cam)))
        _check(N.lib.pt_scene_commit(s, bvh_width))
        info = N.pt_bvh_info()
        _check(N.lib.pt_scene_bvh_info(s, C.byref(info)))
        nodes = np.zeros(max(int(info.node_bytes), 1), np.uint8)
        tris = np.zeros(max(int(info.tri_bytes), 1), np.uint8)
        _check(N.lib.pt_scene_bvh_read(s, _ptr(nodes), info.node_bytes, _ptr(tris), info.tri_bytes))
        return info, nodes[: int(info.node_bytes)], tris[: int(info.tri_bytes)]
    finally:
        N.lib.pt_scene_destroy(s)


def make_params(width, height, spp=1, max_depth=8, rr_start=3, seed=0x5EED0001, mode=N.PT_PATH_TRACE, ray_eps=1e-4,
                rank=0, nranks=1, flags=0, sample_offset=0, streams=1, next_event=False, sphere_lights=False):
    """next_event / sphere_lights: PT_FLAG_NEXT_EVENT (docs/SPEC.md §7) and, with it, PT_FLAG_NEXT_EVENT_SPHERES (§7.1: the scene's emissive
    spheres are lights too), or-ed into `flags`."""
    flags |= (N.PT_FLAG_NEXT_EVENT if next_event else 0) | (N.PT_FLAG_NEXT_EVENT_SPHERES if sphere_lights else 0)
    p = N.pt_render_params()
    p.width, p.height, p.spp, p.max_depth, p.rr_start, p.seed = width, height, spp, max_depth, rr_start, seed
    p.sample_offset, p.mode, p.ray_eps, p.rank, p.nranks, p.tile_size, p.flags = sample_offset, mode, ray_eps, rank, nranks, 0, flags
    p.streams = streams
    return p


def tile_layout(params):
    lay = N.pt_tile_layout()
    _check(N.lib.pt_tile_layout_query(C.byref(params), C.byref(lay)))
    return lay


class _DevicePtr:
    """Exposes a raw device pointer through __cuda_array_interface__ so torch can alias it (no copy)."""

    def __init__(self, ptr, n_floats):
        self.__cuda_array_interface__ = {"shape": (int(n_floats),), "typestr": "<f4", "data": (int(ptr), False), "version": 2}


class Window:
    """Headless stand-in for Silk.NET's IWindow (App.cs:25-33): only the framebuffer size survives; MI355X has no display."""

    def __init__(self, width=1920, height=1080, title="ptrt"):
        self.FramebufferSize = (width, height)
        self.Title = title


class Renderer:
    """Mirror of RayTracing.Graphics.Renderer (Renderer.cs:18-1241), compute path only."""

    def __init__(self, window, device_ordinal=0, stream=None):
        self.Window = window
        self._device = device_ordinal
        self._stream = stream
        self._ctx = C.c_void_p()
        self._scene = C.c_void_p()
        self._disposed = False
        self.Params = make_params(*window.FramebufferSize, mode=N.PT_REFERENCE_SPHERE)
        self.LastStats = N.pt_stats()

    # Renderer.Init (Renderer.cs:66-84): GraphicsDevice.Init + CreateResources + CreateComputePipeline
    def Init(self):
        desc = N.pt_device_desc(self._device, self._stream, 0, 0)
        _check(N.lib.pt_context_create(C.byref(desc), C.byref(self._ctx)))

    def GetTuning(self):
        t = N.pt_tuning()
        _check(N.lib.pt_context_get_tuning(self._ctx, C.byref(t)), self._ctx)
        return t

    def SetTuning(self, **kw):
        """Scheduling knobs of the context (include/ptrt.h pt_tuning: bounces, loops, finish_below, packed_chunk, compact_below,
        sparse_below, sticky_samples, lag). None changes a pixel."""
        t = self.GetTuning()
        for k, v in kw.items():
            if not hasattr(t, k):
                raise AttributeError(f"pt_tuning has no field {k!r}")
            setattr(t, k, v)
        _check(N.lib.pt_context_set_tuning(self._ctx, C.byref(t)), self._ctx)

    def SetScene(self, scene, bvh_width=0):
        """Upload a SceneData and build its BVH (the reference has no scene API; Test.hlsl:6,8,12,13 are literals)."""
        ctx = self._ctx
        if self._scene:
            N.lib.pt_scene_destroy(self._scene)
            self._scene = C.c_void_p()
        _check(N.lib.pt_scene_create(ctx, C.byref(self._scene)), ctx)
        s = self._scene
        verts = np.ascontiguousarray(scene.verts, np.float32)
        tri_mat = np.ascontiguousarray(scene.tri_mat, np.uint32)
        spheres = np.ascontiguousarray(scene.spheres, np.float32)
        sph_mat = np.ascontiguousarray(scene.sph_mat, np.uint32)
        mats = np.ascontiguousarray(scene.mats)
        _check(N.lib.pt_scene_set_triangles(s, _ptr(verts), _ptr(tri_mat), len(tri_mat)), ctx)
        _check(N.lib.pt_scene_set_spheres(s, _ptr(spheres), _ptr(sph_mat), len(sph_mat)), ctx)
        _check(N.lib.pt_scene_set_materials(s, _ptr(mats), len(mats)), ctx)
        _check(N.lib.pt_scene_set_camera(s, C.byref(scene.cam)), ctx)
        sky = (C.c_float * 3)(*[float(v) for v in scene.sky])
        _check(N.lib.pt_scene_set_sky(s, C.byref(sky)), ctx)
        if getattr(scene, "environment", None) is not None:
            self.SetEnvironment(scene.environment)
        self._set_textures(scene)
        _check(N.lib.pt_scene_commit(s, bvh_width), ctx)

    def _set_textures(self, scene):
        """docs/SPEC.md §13: a SceneData's uvs, textures and material_textures, before the commit that makes them take effect."""
        s, ctx = self._scene, self._ctx
        if getattr(scene, "uvs", None) is not None:
            uv = np.ascontiguousarray(scene.uvs, np.float32).reshape(-1, 6)
            _check(N.lib.pt_scene_set_triangle_uvs(s, _ptr(uv), len(uv)), ctx)
        for index, t in sorted((getattr(scene, "textures", None) or {}).items()):
            img, flags = t if isinstance(t, tuple) else (t, 0)
            a = np.ascontiguousarray(img, np.float32)
            if a.ndim != 3 or a.shape[2] != 3:
                raise ValueError(f"texture {index} must be H x W x 3, got {a.shape}")
            _check(N.lib.pt_scene_set_texture(s, index, _ptr(a), a.shape[1], a.shape[0], flags), ctx)
        if getattr(scene, "material_textures", None) is not None:
            mt = np.ascontiguousarray(scene.material_textures, np.uint32)
            _check(N.lib.pt_scene_set_material_textures(s, _ptr(mt), len(mt)), ctx)

    def SetTriangleUVs(self, uvs):
        """(triangles, 6) per-triangle UVs of the current scene, or None to remove them; takes effect with the next Commit()."""
        uv = None if uvs is None else np.ascontiguousarray(uvs, np.float32).reshape(-1, 6)
        _check(N.lib.pt_scene_set_triangle_uvs(self._scene, _ptr(uv), 0 if uv is None else len(uv)), self._ctx)

    def SetTexture(self, index, img, flags=0):
        """Texture `index` of the current scene: H x W x 3 linear RGB, or None to remove it; takes effect with the next Commit()."""
        if img is None:
            _check(N.lib.pt_scene_set_texture(self._scene, index, None, 0, 0, 0), self._ctx)
            return
        a = np.ascontiguousarray(img, np.float32)
        if a.ndim != 3 or a.shape[2] != 3:
            raise ValueError(f"texture {index} must be H x W x 3, got {a.shape}")
        _check(N.lib.pt_scene_set_texture(self._scene, index, _ptr(a), a.shape[1], a.shape[0], flags), self._ctx)

    def SetMaterialTextures(self, texture_of_material):
        """One texture index or native.PT_NO_TEXTURE per material, or None to remove the binding; takes effect with the next Commit()."""
        mt = None if texture_of_material is None else np.ascontiguousarray(texture_of_material, np.uint32)
        _check(N.lib.pt_scene_set_material_textures(self._scene, _ptr(mt), 0 if mt is None else len(mt)), self._ctx)

    def Commit(self, bvh_width=0):
        """pt_scene_commit of the current scene: what the setters above changed takes effect."""
        _check(N.lib.pt_scene_commit(self._scene, bvh_width), self._ctx)

    def TextureInfo(self, index):
        """pt_texture_info of texture `index` of the current scene (width 0: not set)."""
        info = N.pt_texture_info()
        _check(N.lib.pt_scene_texture_info(self._scene, index, C.byref(info)), self._ctx)
        return info

    def SetEnvironment(self, rgb):
        """Give the current scene an environment map (include/ptrt.h pt_scene_set_environment: n x n x 3 floats, octahedral layout,
        docs/SPEC.md §11; no new commit needed), or remove it with None."""
        if rgb is None:
            _check(N.lib.pt_scene_set_environment(self._scene, None, 0), self._ctx)
            return
        a = np.ascontiguousarray(rgb, np.float32)
        if a.ndim != 3 or a.shape[0] != a.shape[1] or a.shape[2] != 3:
            raise ValueError(f"environment must be n x n x 3, got {a.shape}")
        _check(N.lib.pt_scene_set_environment(self._scene, _ptr(a), a.shape[0]), self._ctx)

    def EnvironmentInfo(self):
        info = N.pt_environment_info()
        _check(N.lib.pt_scene_environment_info(self._scene, C.byref(info)), self._ctx)
        return info

    def SetLens(self, radius, focus_distance):
        """Give the current scene a thin lens (include/ptrt.h pt_scene_set_lens, docs/SPEC.md §3.1: depth of field; no new commit
        needed). radius 0 is the pinhole. A caller that changes the lens restarts accumulation."""
        lens = N.pt_lens(radius=radius, focus_distance=focus_distance)
        _check(N.lib.pt_scene_set_lens(self._scene, C.byref(lens)), self._ctx)

    def ClearLens(self):
        _check(N.lib.pt_scene_set_lens(self._scene, None), self._ctx)

    def Lens(self):
        """(radius, focus_distance) of the current scene's lens; (0.0, 0.0) when none is set."""
        lens = N.pt_lens()
        _check(N.lib.pt_scene_get_lens(self._scene, C.byref(lens)), self._ctx)
        return lens.radius, lens.focus_distance

    def SetCamera(self, cam):
        """Move the current scene's camera (include/ptrt.h pt_scene_set_camera: no new commit needed)."""
        _check(N.lib.pt_scene_set_camera(self._scene, C.byref(cam)), self._ctx)

    def BvhInfo(self):
        info = N.pt_bvh_info()
        _check(N.lib.pt_scene_bvh_info(self._scene, C.byref(info)), self._ctx)
        return info

    def BvhRead(self):
        """(nodes bytes, tris48 bytes) of the SPEC §4.1 blob, for a checker that wants to traverse the same bytes."""
        info = self.BvhInfo()
        nodes = np.zeros(max(int(info.node_bytes), 1), np.uint8)
        tris = np.zeros(max(int(info.tri_bytes), 1), np.uint8)
        _check(N.lib.pt_scene_bvh_read(self._scene, _ptr(nodes), info.node_bytes, _ptr(tris), info.tri_bytes), self._ctx)
        return nodes[: int(info.node_bytes)], tris[: int(info.tri_bytes)]

    def TraceRays(self, rays, tmax=None, occlusion=False, count_visits=False):
        """Ray queries on the current scene (include/ptrt.h pt_trace_rays, docs/SPEC.md §4.2); returns (hits, pt_stats).

        rays: an (N, 8) float32 array of {o.xyz, tmax, d.xyz, 0} records, or a pair (origins, directions) of (N, 3) arrays (|d| = 1
        for spheres). tmax: None keeps the records' own column (+inf for a pair), else a scalar or (N,) array that replaces it.
        torch tensors on the renderer's device are passed as device pointers (an (N, 8) contiguous float32 tensor without tmax is
        used in place); numpy arrays take the staged host path. hits: (N, 4) float32 of the same kind, {t, prim id bits, u, v}; a miss
        is {+inf, 0xFFFFFFFF, 0, 0} — `hits[:, 1].view(np.uint32)` (torch: `.view(torch.int32)`) gives the ids."""
        pair = isinstance(rays, (tuple, list))
        first = rays[0] if pair else rays
        flags = (N.PT_TRACE_OCCLUSION if occlusion else 0) | (N.PT_TRACE_COUNT_VISITS if count_visits else 0)
        stats = N.pt_stats()
        if N.torch is not None and isinstance(first, N.torch.Tensor):
            torch = N.torch
            dev = first.device
            if dev.type != "cuda" or (dev.index if dev.index is not None else torch.cuda.current_device()) != self._device:
                raise ValueError(f"rays are on {dev}, the renderer on cuda:{self._device}")
            if pair:
                o, d = (torch.as_tensor(a, dtype=torch.float32, device=dev).reshape(-1, 3) for a in rays)
                rec = torch.cat([o, torch.full_like(o[:, :1], float("inf")), d, torch.zeros_like(o[:, :1])], dim=1)
            else:
                rec = rays if rays.dtype == torch.float32 and rays.is_contiguous() and rays.dim() == 2 and rays.shape[1] == 8 else \
                    rays.to(torch.float32).reshape(-1, 8).contiguous()
            if tmax is not None:
                rec = rec if pair else rec.clone()  # never write into the caller's tensor
                rec[:, 3] = torch.as_tensor(tmax, dtype=torch.float32, device=dev)
            hits = torch.empty((rec.shape[0], 4), dtype=torch.float32, device=dev)
            if rec.shape[0] == 0:  # (an empty tensor has no storage to point at)
                return hits, stats
            torch.cuda.current_stream(dev).synchronize()  # the library runs on its own stream: the records must be complete
            _check(N.lib.pt_trace_rays(self._ctx, self._scene, C.c_void_p(rec.data_ptr()), C.c_void_p(hits.data_ptr()),
                                       rec.shape[0], flags, C.byref(stats)), self._ctx)
            return hits, stats
        if pair:
            o, d = (np.asarray(a, np.float32).reshape(-1, 3) for a in rays)
            rec = np.zeros((len(o), 8), np.float32)
            rec[:, 0:3], rec[:, 3], rec[:, 4:7] = o, np.inf, d
        else:
            rec = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        if tmax is not None:
            rec = rec if pair else rec.copy()  # never write into the caller's array
            rec[:, 3] = tmax
        hits = np.empty((len(rec), 4), np.float32)
        _check(N.lib.pt_trace_rays(self._ctx, self._scene, _ptr(rec), _ptr(hits), len(rec), flags | N.PT_TRACE_HOST_MEMORY,
                                   C.byref(stats)), self._ctx)
        return hits, stats

    def Gather(self, points, normals, samples=64, seed=0, sample_offset=0, point_offset=0, max_distance=0.0, ray_eps=1e-3):
        """Hemisphere gathers at surface points of the current scene (include/ptrt.h pt_gather, docs/SPEC.md §12): ambient occlusion, sky
        irradiance and the bent normal of a bake; returns (E, visibility, bent, pt_stats).

        points, normals: (N, 3) positions and (not necessarily unit) normals. float32 torch tensors on the renderer's device go in as
        device pointers and the results are tensors on that device (the current stream is synchronised first); numpy arrays take the
        staged host path. E: (N, 3), the mean radiance of the unoccluded directions (pi * E = irradiance from the sky or the
        environment map); visibility: (N,), the unoccluded share of the `samples` cosine-weighted directions (1 - ambient occlusion; -1
        marks an invalid point); bent: (N, 3), the mean unoccluded direction, not normalised."""
        gp = N.pt_gather_params(samples=samples, seed=seed, sample_offset=sample_offset, point_offset=point_offset,
                                max_distance=max_distance, ray_eps=ray_eps, flags=0)
        return self._gather(points, normals, gp, lambda *a: N.lib.pt_gather(*a))

    def GatherPaths(self, points, normals, samples=64, seed=0, sample_offset=0, point_offset=0, max_distance=0.0, ray_eps=1e-3,
                    max_depth=8, rr_start=3, next_event=False, sphere_lights=False):
        """Path-traced gathers (include/ptrt.h pt_gather_paths, docs/SPEC.md §12.1): Gather's points, arguments and results, with every
        sample a whole path of at most `max_depth` segments (Russian roulette from depth `rr_start` on) that starts at the point. E is
        the mean radiance the paths bring — emissive surfaces and bounced light included, so pi * E is a Lambert texel's irradiance in
        a closed, emitter-lit scene too; visibility and bent are Gather's. The pt_stats' rays are the path segments traced.
        next_event (PT_GATHER_PATHS_NEXT_EVENT, §12.2): every sample also samples the scene's lights (emissive triangles, a lit
        environment map) at the point and at its Lambert vertices, with multiple importance sampling — the same expectation with less
        noise under small lights, and with max_depth = 1 a direct-light bake; rays then counts the shadow rays too.
        sphere_lights (PT_GATHER_PATHS_SPHERE_LIGHTS, §7.1; needs next_event): the scene's emissive spheres are lights too, sampled by
        the cone they subtend."""
        gp = N.pt_gather_params(samples=samples, seed=seed, sample_offset=sample_offset, point_offset=point_offset,
                                max_distance=max_distance, ray_eps=ray_eps, flags=0)
        pp = N.pt_gather_path_params(max_depth=max_depth, rr_start=rr_start, flags=(N.PT_GATHER_PATHS_NEXT_EVENT if next_event else 0) | (N.PT_GATHER_PATHS_SPHERE_LIGHTS if sphere_lights else 0))
        return self._gather(points, normals, gp, lambda *a: N.lib.pt_gather_paths(*a[:-1], C.byref(pp), a[-1]))

    def _gather(self, points, normals, gp, call):
        """Gather / GatherPaths: builds the records, calls call(ctx, scene, points, out, n, gp, stats), splits the rows."""
        stats = N.pt_stats()
        if N.torch is not None and isinstance(points, N.torch.Tensor):
            torch = N.torch
            dev = points.device
            if dev.type != "cuda" or (dev.index if dev.index is not None else torch.cuda.current_device()) != self._device:
                raise ValueError(f"points are on {dev}, the renderer on cuda:{self._device}")
            p, n = (torch.as_tensor(a, dtype=torch.float32, device=dev).reshape(-1, 3) for a in (points, normals))
            if p.shape != n.shape:
                raise ValueError(f"{p.shape[0]} points, {n.shape[0]} normals")
            zero = torch.zeros_like(p[:, :1])
            rec = torch.cat([p, zero, n, zero], dim=1)
            out = torch.empty((rec.shape[0], 8), dtype=torch.float32, device=dev)
            if rec.shape[0]:  # (an empty tensor has no storage to point at)
                torch.cuda.current_stream(dev).synchronize()  # the library runs on its own stream: the records must be complete
                _check(call(self._ctx, self._scene, C.c_void_p(rec.data_ptr()), C.c_void_p(out.data_ptr()), rec.shape[0],
                            C.byref(gp), C.byref(stats)), self._ctx)
            return out[:, 0:3], out[:, 3], out[:, 4:7], stats
        p, n = (np.asarray(a, np.float32).reshape(-1, 3) for a in (points, normals))
        if p.shape != n.shape:
            raise ValueError(f"{p.shape[0]} points, {n.shape[0]} normals")
        rec = np.zeros((len(p), 8), np.float32)
        rec[:, 0:3], rec[:, 4:7] = p, n
        out = np.empty((len(rec), 8), np.float32)
        gp.flags = N.PT_GATHER_HOST_MEMORY
        _check(call(self._ctx, self._scene, _ptr(rec), _ptr(out), len(rec), C.byref(gp), C.byref(stats)), self._ctx)
        return out[:, 0:3], out[:, 3], out[:, 4:7], stats

    def UpdateGeometry(self, verts=None, spheres=None):
        """Move the current scene's triangles and/or spheres without a new commit (include/ptrt.h pt_scene_update_triangles /
        pt_scene_update_spheres, docs/SPEC.md §4.3); returns the triangle update's pt_stats (gpu_ms), zeros without one.

        verts: (N, 9) or (N, 3, 3) float32, the committed count and order; a float32 torch tensor on the renderer's device goes in as a
        device pointer (the current stream is synchronised first), numpy arrays take the staged host path. spheres: (S, 4) centres
        and radii, the committed count (host memory). The tree keeps its topology, so the picture is exactly that of a fresh SetScene
        of the moved geometry; BvhInfo().sah_cost tells how much the old tree has degraded. Each of the two is one library call:
        the triangles are updated first, and a refused sphere update leaves the triangle update in place."""
        stats = N.pt_stats()
        if verts is not None:
            if N.torch is not None and isinstance(verts, N.torch.Tensor):
                torch = N.torch
                dev = verts.device
                if dev.type != "cuda" or (dev.index if dev.index is not None else torch.cuda.current_device()) != self._device:
                    raise ValueError(f"verts are on {dev}, the renderer on cuda:{self._device}")
                v = verts.to(torch.float32).reshape(-1, 9).contiguous()
                torch.cuda.current_stream(dev).synchronize()  # the library runs on its own stream: the vertices must be complete
                _check(N.lib.pt_scene_update_triangles(self._scene, C.c_void_p(v.data_ptr() if v.shape[0] else None), v.shape[0], 0,
                                                       C.byref(stats)), self._ctx)
            else:
                v = np.ascontiguousarray(verts, np.float32).reshape(-1, 9)
                _check(N.lib.pt_scene_update_triangles(self._scene, _ptr(v), len(v), N.PT_UPDATE_HOST_MEMORY, C.byref(stats)), self._ctx)
        if spheres is not None:
            if N.torch is not None and isinstance(spheres, N.torch.Tensor):
                spheres = spheres.detach().cpu().numpy()
            sph = np.ascontiguousarray(spheres, np.float32).reshape(-1, 4)
            _check(N.lib.pt_scene_update_spheres(self._scene, _ptr(sph), len(sph)), self._ctx)
        return stats

    def Denoise(self, iterations=0, sigma_color=0.0, sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0, guides_only=False,
                edge_stops=True):
        """Denoise the last assembled frame with guides traced on the current scene (include/ptrt.h pt_denoise, docs/SPEC.md §8);
        returns pt_stats (rays = guide rays, extend_ms = guide pass, other_ms = filter passes). Zeros mean the defaults. The frame
        itself (ReadFramebuffer, accumulated sums) is not touched; ReadDenoised / ReadGuides hold until the next Render."""
        dp = N.pt_denoise_params(iterations, sigma_color, sigma_normal, sigma_depth, sigma_albedo,
                                 (N.PT_DENOISE_GUIDES_ONLY if guides_only else 0) | (0 if edge_stops else N.PT_DENOISE_NO_EDGE_STOPS))
        stats = N.pt_stats()
        _check(N.lib.pt_denoise(self._ctx, self._scene, C.byref(dp), C.byref(stats)), self._ctx)
        return stats

    def ReadDenoised(self):
        """The denoised frame, (H, W, 4) float32 (alpha as in the framebuffer)."""
        w, h = self.Params.width, self.Params.height
        out = np.empty((h, w, 4), np.float32)
        _check(N.lib.pt_denoised_read(self._ctx, _ptr(out), out.size), self._ctx)
        return out

    def ReadGuides(self):
        """The guide buffers of the last Denoise, (H, W, 8) float32: front-facing normal, t, albedo, prim id bits
        (`[..., 7].view(np.uint32)`; a miss is t = +inf, id 0xFFFFFFFF). What a host's own denoiser takes as features."""
        w, h = self.Params.width, self.Params.height
        out = np.empty((h, w, 8), np.float32)
        _check(N.lib.pt_guides_read(self._ctx, _ptr(out), out.size), self._ctx)
        return out

    def DenoiseTemporal(self, max_history=0, plane_tolerance=0.0, normal_min=0.0, reset=False, match_ids=False, filter=True, motion=False,
                        **denoise):
        """Temporal accumulation (include/ptrt.h pt_denoise_temporal, docs/SPEC.md §9): reproject the previous call's accumulated image
        to the last rendered frame through the two cameras and the first-hit guides, blend the frame in, keep the result as the next
        history, and — with `filter` — run Denoise's filter over it (`denoise`: Denoise's keyword arguments). Zeros mean the defaults.
        Returns pt_stats (paths = pixels that took history, shade_ms = the temporal pass). ReadTemporal / ReadHistoryLength /
        ReadDenoised / ReadGuides hold until the next Render; the history lives in the context until `reset` or a change of size.
        `motion` (PT_TEMPORAL_MOTION, §9.1): the call also records the geometry it was traced on, and a pixel whose primitive
        UpdateGeometry has moved since the previous `motion` call takes its history from where its surface point was;
        stats.reserved[0] = pixels of moved primitives."""
        tp = N.pt_temporal_params(max_history, plane_tolerance, normal_min,
                                  (N.PT_TEMPORAL_RESET if reset else 0) | (N.PT_TEMPORAL_MATCH_IDS if match_ids else 0)
                                  | (N.PT_TEMPORAL_MOTION if motion else 0))
        dp = None
        if filter:
            dp = N.pt_denoise_params(denoise.pop("iterations", 0), denoise.pop("sigma_color", 0.0), denoise.pop("sigma_normal", 0.0),
                                     denoise.pop("sigma_depth", 0.0), denoise.pop("sigma_albedo", 0.0),
                                     (N.PT_DENOISE_GUIDES_ONLY if denoise.pop("guides_only", False) else 0)
                                     | (0 if denoise.pop("edge_stops", True) else N.PT_DENOISE_NO_EDGE_STOPS))
        if denoise:
            raise TypeError(f"DenoiseTemporal: unknown arguments {sorted(denoise)}")
        stats = N.pt_stats()
        _check(N.lib.pt_denoise_temporal(self._ctx, self._scene, C.byref(tp), C.byref(dp) if dp is not None else None, C.byref(stats)),
               self._ctx)
        return stats

    def ReadTemporal(self):
        """The accumulated image of the last DenoiseTemporal, (H, W, 4) float32 (alpha as in the framebuffer), before any filter."""
        w, h = self.Params.width, self.Params.height
        out = np.empty((h, w, 4), np.float32)
        _check(N.lib.pt_temporal_read(self._ctx, _ptr(out), out.size), self._ctx)
        return out

    def ReadHistoryLength(self):
        """(H, W) float32: how many frames each pixel's accumulated colour stands for (1 = it took no history)."""
        w, h = self.Params.width, self.Params.height
        out = np.empty((h, w), np.float32)
        _check(N.lib.pt_temporal_history_read(self._ctx, _ptr(out), out.size), self._ctx)
        return out

    _DISPLAY_SOURCES = {"frame": N.PT_DISPLAY_FRAME, "denoised": N.PT_DISPLAY_DENOISED, "temporal": N.PT_DISPLAY_TEMPORAL}
    _TONE_CURVES = {"clamp": N.PT_TONE_CLAMP, "reinhard": N.PT_TONE_REINHARD, "aces": N.PT_TONE_ACES}

    def Display(self, source="frame", curve="clamp", exposure=0.0, auto=False, white=0.0, key=0.0, adapt=0.0, trim_low=0, trim_high=0,
                linear=False, reset=False):
        """The display stage (include/ptrt.h pt_display, docs/SPEC.md §10) — what stands where the reference's display pass samples the
        image (Renderer.cs:1042-1121): the frame, the denoised or the accumulated image times an exposure, through a tone curve, encoded
        to sRGB8 (`linear`: UNORM8) on the device. `auto` meters the exposure from a luminance histogram (`key`, `trim_*` per mille)
        and moves `adapt` of the way from the previous call's exposure to it; `exposure` then compensates on top. Zeros mean the
        defaults. Returns pt_stats (extend_ms = metering, other_ms = tone pass). ReadDisplay / DisplayInfo / ReadDisplayHistogram hold
        until the next Render; the adapted exposure lives in the context until `reset`."""
        dp = N.pt_display_params(self._DISPLAY_SOURCES[source], self._TONE_CURVES[curve], exposure, white, key, adapt, trim_low, trim_high,
                                 (N.PT_DISPLAY_AUTO_EXPOSURE if auto else 0) | (N.PT_DISPLAY_LINEAR if linear else 0)
                                 | (N.PT_DISPLAY_RESET_ADAPTATION if reset else 0))
        stats = N.pt_stats()
        _check(N.lib.pt_display(self._ctx, C.byref(dp), C.byref(stats)), self._ctx)
        return stats

    def ReadDisplay(self):
        """The displayed image of the last Display, (H, W, 4) uint8 in RGBA order."""
        w, h = self.Params.width, self.Params.height
        out = np.empty((h, w, 4), np.uint8)
        _check(N.lib.pt_display_read(self._ctx, _ptr(out), out.size), self._ctx)
        return out

    def DisplayInfo(self):
        """pt_display_info of the last Display: the exposure applied, the metered one, the log-average luminance, the pixel counts."""
        info = N.pt_display_info()
        _check(N.lib.pt_display_info_read(self._ctx, C.byref(info)), self._ctx)
        return info

    def ReadDisplayHistogram(self):
        """The 512 luminance bins the last Display metered (uint32; 8 bins per octave from 2^-32; all 0 without `auto`)."""
        out = np.empty(512, np.uint32)
        _check(N.lib.pt_display_histogram_read(self._ctx, _ptr(out), out.size), self._ctx)
        return out

    # Renderer.Update (Renderer.cs:86-89) is empty in the reference
    def Update(self, deltaTime):
        pass

    # Renderer.Render (Renderer.cs:933-1004): [acquire] -> ComputeFrame -> wait fence -> [draw, present]
    def Render(self, delta):
        self.ComputeFrame(delta)
        return self.LastStats

    # Renderer.ComputeFrame (Renderer.cs:1006-1040). `delta` is unused there too.
    def ComputeFrame(self, delta):
        scene = self._scene if self.Params.mode == N.PT_PATH_TRACE else None
        stats = N.pt_stats()  # a fresh object per frame: callers keep the stats of earlier frames
        _check(N.lib.pt_render(self._ctx, scene, C.byref(self.Params), C.byref(stats)), self._ctx)
        self.LastStats = stats

    def ReadFramebuffer(self):
        w, h = self.Params.width, self.Params.height
        out = np.empty((h, w, 4), np.float32)
        _check(N.lib.pt_framebuffer_read(self._ctx, _ptr(out), out.size), self._ctx)
        return out

    def ReadFramebufferRGBA8(self):
        w, h = self.Params.width, self.Params.height
        out = np.empty((h, w, 4), np.uint8)
        _check(N.lib.pt_framebuffer_read_rgba8(self._ctx, _ptr(out), out.size), self._ctx)
        return out

    def ReadFramebufferSRGB8(self):
        """The frame as the reference's window would show it (UNORM8 image -> B8G8R8A8Srgb swapchain, SwapChain.cs:157-158)."""
        w, h = self.Params.width, self.Params.height
        out = np.empty((h, w, 4), np.uint8)
        _check(N.lib.pt_framebuffer_read_srgb8(self._ctx, _ptr(out), out.size), self._ctx)
        return out

    def SaveImage(self, path, srgb=False, display=False):
        """Image output — what replaces the reference's window (display path Renderer.cs:1042-1121).
        `.ppm`: 8-bit, the clamp-and-round R8G8B8A8Unorm image of Renderer.cs:124 — or, with srgb=True, what the reference's
        sRGB swapchain shows of it (SwapChain.cs:157-158; no tone mapping, values above 1 clip) — or, with display=True, the image
        of the last Display (exposed, tone-mapped, encoded from the floats); `.pfm`: linear float radiance, bottom-up rows."""
        w, h = self.Params.width, self.Params.height
        if path.lower().endswith(".pfm"):
            rgb = np.ascontiguousarray(self.ReadFramebuffer()[::-1, :, :3], "<f4")
            with open(path, "wb") as f:
                f.write(b"PF\n%d %d\n-1.0\n" % (w, h))
                f.write(rgb.tobytes())
        else:
            img = self.ReadDisplay() if display else self.ReadFramebufferSRGB8() if srgb else self.ReadFramebufferRGBA8()
            rgb = np.ascontiguousarray(img[..., :3])
            with open(path, "wb") as f:
                f.write(b"P6\n%d %d\n255\n" % (w, h))
                f.write(rgb.tobytes())

    def TilesDevice(self):
        """Device view (for torch.as_tensor) of this rank's tile-major radiance sums after a frame."""
        ptr, n = C.c_void_p(), C.c_uint64()
        _check(N.lib.pt_tiles_device_ptr(self._ctx, C.byref(ptr), C.byref(n)), self._ctx)
        return _DevicePtr(ptr.value, n.value)

    def AssembleTiles(self, gathered_ptr, n_floats):
        _check(N.lib.pt_assemble_tiles(self._ctx, C.byref(self.Params), C.c_void_p(gathered_ptr), n_floats), self._ctx)

    # IDisposable pattern (Renderer.cs:1192-1216, 1235-1240)
    def Dispose(self):
        if self._disposed:
            return
        if self._scene:
            N.lib.pt_scene_destroy(self._scene)
            self._scene = C.c_void_p()
        if self._ctx:
            N.lib.pt_context_destroy(self._ctx)
            self._ctx = C.c_void_p()
        self._disposed = True

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.Dispose()

    def __del__(self):
        try:
            self.Dispose()
        except Exception:
            pass


class Comm:
    """Several ranks of one frame behind one call (include/ptrt.h pt_comm): one Renderer per rank on its own GPU (tiles exchanged by
    one ncclGather per frame inside libptrt), or the same Renderer for every rank (virtual ranks rendered one after the other: the
    partition rehearsed on a single GPU). Every renderer must hold the same scene. The frame lands in renderers[root]."""

    def __init__(self, renderers, root=0, flags=0):
        self.Renderers = list(renderers)
        self.Root = root
        self._comm = C.c_void_p()
        ctxs = (C.c_void_p * len(self.Renderers))(*[r._ctx for r in self.Renderers])
        _check(N.lib.pt_comm_create(ctxs, len(self.Renderers), root, flags, C.byref(self._comm)))

    def Render(self, params):
        """One frame of `params` over all ranks; returns the per-rank pt_stats."""
        n = len(self.Renderers)
        scenes = (C.c_void_p * n)(*[r._scene for r in self.Renderers])
        stats = (N.pt_stats * n)()
        _check(N.lib.pt_comm_render(self._comm, scenes, C.byref(params), stats), self.Renderers[self.Root]._ctx)
        self.Renderers[self.Root].Params = params
        return list(stats)

    def StageTiles(self, rank):
        _check(N.lib.pt_comm_stage_tiles(self._comm, rank), self.Renderers[self.Root]._ctx)

    def Assemble(self, params):
        _check(N.lib.pt_comm_assemble(self._comm, C.byref(params)), self.Renderers[self.Root]._ctx)
        self.Renderers[self.Root].Params = params

    def Dispose(self):
        if self._comm:
            N.lib.pt_comm_destroy(self._comm)
            self._comm = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.Dispose()


class App:
    """Mirror of RayTracing.App (App.cs:7-68): Run() = InitWindow -> InitRenderer -> render loop."""

    def __init__(self, frames=1, width=1920, height=1080, device_ordinal=0):
        self.Window = None
        self.Renderer = None
        self._frames = frames
        self._size = (width, height)
        self._device = device_ordinal
        self._disposed = False

    def Run(self):
        self.InitWindow()
        self.InitRenderer()
        for _ in range(self._frames):  # Window.Run() -> Render event (App.cs:20,39-42)
            self.Renderer.Render(0.0)

    def InitWindow(self):
        self.Window = Window(*self._size)  # App.cs:25-29: 1920 x 1080

    def InitRenderer(self):
        self.Renderer = Renderer(self.Window, self._device)
        self.Renderer.Init()

    def Dispose(self):
        if not self._disposed:
            if self.Renderer is not None:
                self.Renderer.Dispose()
            self._disposed = True

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.Dispose()
