"""Shared by the temporal tests (tests/test_temporal.py, tests/test_gpu_temporal.py) and tools/exp_temporal.py: camera motion, the
camera path of the quality experiment, a float64 reprojection, hand-built scenes and the displayed error. Test infrastructure only."""
import ctypes as C
import dataclasses

import numpy as np


def copy_camera(cam):
    c = type(cam)()
    C.memmove(C.byref(c), C.byref(cam), C.sizeof(cam))
    return c


def move_camera(cam, along_right=0.0, yaw_deg=0.0, offset=(0.0, 0.0, 0.0)):
    """A copy of `cam` translated by `along_right` along its unit right vector plus `offset`, then yawed by `yaw_deg` about its unit up
    vector (forward and right turn, their lengths stay)."""
    c = copy_camera(cam)
    o, f, r, u = (np.array(v[:], np.float64) for v in (cam.origin, cam.forward, cam.right, cam.up))
    o = o + along_right * r / np.linalg.norm(r) + np.asarray(offset, np.float64)
    k, a = u / np.linalg.norm(u), np.radians(yaw_deg)

    def rot(v):
        return v * np.cos(a) + np.cross(k, v) * np.sin(a) + k * np.dot(k, v) * (1.0 - np.cos(a))

    f, r = rot(f), rot(r)
    c.origin[:], c.forward[:], c.right[:] = o.tolist(), f.tolist(), r.tolist()
    return c


def camera_path(cam, frames=8, step=0.01, yaw_deg=0.3):
    """The quality experiment's path: frame k has moved k * step along `right` and yawed k * yaw_deg."""
    return [move_camera(cam, k * step, k * yaw_deg) for k in range(frames)]


def with_camera(sd, cam):
    return dataclasses.replace(sd, cam=cam)


def world_positions64(pto, cam, g8):
    """float64 world position of every pixel's first hit from the f32 camera rays and guide depths (misses: inf / nan)."""
    h, w = g8.shape[:2]
    c = copy_camera(cam)
    c.jitter = 0
    P = np.zeros((h, w, 3))
    for y in range(h):
        for x in range(w):
            o, d = pto.camera_ray(c, x, y)
            P[y, x] = o.astype(np.float64) + np.float64(g8[y, x, 3]) * d.astype(np.float64)
    return P


def reproject64(old_cam, P):
    """float64 pixel coordinates (fx, fy) of world positions P (h, w, 3) in the image of `old_cam`, and whether they lie in front of it:
    wv = alpha * (f + sx r + sy u) solved as a 3 x 3 system, then the inverse of §3's pixel -> (sx, sy) map."""
    o, f, r, u = (np.array(v[:], np.float64) for v in (old_cam.origin, old_cam.forward, old_cam.right, old_cam.up))
    M = np.stack([f, r, u], axis=1)
    with np.errstate(all="ignore"):
        sol = np.linalg.solve(M, (P - o).reshape(-1, 3).T).T.reshape(P.shape)
        alpha = sol[..., 0]
        sx, sy = sol[..., 1] / alpha, sol[..., 2] / alpha
        fx = (sx + np.float64(old_cam.cx)) / np.float64(old_cam.scale) - 0.5
        fy = (sy + np.float64(old_cam.cy)) / np.float64(old_cam.scale) - 0.5
    return fx, fy, alpha > 0


def axis_camera(P, w, h, origin=(0.0, 0.0, 0.0), jitter=0):
    """A camera at `origin` looking down -z with a 90 degree vertical field of view."""
    cam = P.native.pt_camera()
    cam.origin[:] = origin
    cam.forward[:], cam.right[:], cam.up[:] = (0.0, 0.0, -1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)
    cam.scale, cam.cx, cam.cy, cam.jitter = 2.0 / h, w / h, 1.0, jitter
    return cam


def quad(x0, x1, y0, y1, z):
    """Two triangles facing +z."""
    return [[x0, y0, z, x1, y0, z, x1, y1, z], [x0, y0, z, x1, y1, z, x0, y1, z]]


def wall_and_quad(P, w, h, quad_x=-1.0, cam=None):
    """A wall at z = -3 (triangles 0, 1) and a 0.8 x 1.0 quad in front of it at z = -2 (triangles 2, 3) whose left edge is at quad_x."""
    sd = P.SceneData()
    sd.verts = np.array(quad(-6.0, 6.0, -5.0, 5.0, -3.0) + quad(quad_x, quad_x + 0.8, -0.5, 0.5, -2.0), np.float32)
    sd.tri_mat = np.array([0, 0, 1, 1], np.uint32)
    sd.mats = np.zeros(2, P.MATERIAL_DTYPE)
    sd.mats["albedo"] = [(0.7, 0.7, 0.7), (0.8, 0.3, 0.2)]
    sd.cam = cam if cam is not None else axis_camera(P, w, h)
    return sd


def display_rmse(a, ref):
    """RMSE of the displayed image: radiance clamped to [0, 1], what the 8-bit framebuffer shows (SPEC §1 unorm8)."""
    return float(np.sqrt(np.mean((np.clip(a[..., :3].astype(np.float64), 0, 1) - np.clip(ref[..., :3].astype(np.float64), 0, 1)) ** 2)))


def linear_rmse(a, ref):
    return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - ref[..., :3].astype(np.float64)) ** 2)))


def device_quality(P, r, kind, w, h, frames=8, ref_spp=4096, **temporal):
    """The quality experiment on the device: `frames` 1-spp frames with their own seeds along camera_path, each followed by a
    DenoiseTemporal with the default filter; then pt_denoise alone on the last frame; errors against a ref_spp frame at the last camera.
    Returns {"display": (filter alone, temporal + filter), "linear": (...), "took": fraction of pixels with history in the last call}."""
    sd = P.make_scene(kind, 0, 3, w, h)
    r.SetScene(sd, 0)
    cams = camera_path(sd.cam, frames)
    for k, cam in enumerate(cams):
        r.SetCamera(cam)
        r.Params = P.make_params(w, h, spp=1, max_depth=8, seed=1000 + k)
        r.Render(0.0)
        st = r.DenoiseTemporal(reset=k == 0, **temporal)
    both = r.ReadDenoised()
    r.Denoise()
    alone = r.ReadDenoised()
    r.Params = P.make_params(w, h, spp=ref_spp, max_depth=8, seed=99, streams=8)
    r.Render(0.0)
    ref = r.ReadFramebuffer()
    return {"display": (display_rmse(alone, ref), display_rmse(both, ref)), "linear": (linear_rmse(alone, ref), linear_rmse(both, ref)),
            "took": st.paths / float(w * h)}
