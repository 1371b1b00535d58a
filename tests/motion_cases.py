"""Shared by the motion tests (tests/test_gpu_temporal_motion.py) and tools/exp_temporal_motion.py: a triangle object to animate inside
the generator's scenes, its motions, and the quality experiment of DESIGN.md §12.1 on the device and on the oracle's frames. Test
infrastructure only."""
import dataclasses

import numpy as np

import temporal_cases as tc


def with_object(P, sd, centre=(0.05, -0.1, 0.2), size=1.0, tilt_deg=20.0, lean_deg=0.0):
    """`sd` plus a square of two triangles (the last two ids) of its own material, facing the camera side (+z), tilted about y and
    leaning back by lean_deg (its face turns up, towards Cornell's ceiling light)."""
    c, a, b, s = np.asarray(centre, np.float64), np.radians(tilt_deg), np.radians(lean_deg), size / 2
    ux, uy = np.array([np.cos(a), 0.0, -np.sin(a)]) * s, np.array([0.0, np.cos(b), -np.sin(b)]) * s
    p = [c - ux - uy, c + ux - uy, c + ux + uy, c - ux + uy]
    tris = np.array([np.concatenate([p[0], p[1], p[2]]), np.concatenate([p[0], p[2], p[3]])], np.float32)
    mats = np.zeros(len(sd.mats) + 1, sd.mats.dtype)
    mats[:-1] = sd.mats
    mats[-1]["albedo"] = (0.75, 0.45, 0.2)
    if "ior" in mats.dtype.names:
        mats[-1]["ior"] = 1.0
    return dataclasses.replace(sd, verts=np.concatenate([np.asarray(sd.verts, np.float32).reshape(-1, 9), tris]),
                               tri_mat=np.concatenate([sd.tri_mat, np.array([len(sd.mats)] * 2, np.uint32)]), mats=mats)


def object_ids(sd):
    n = len(sd.tri_mat)
    return n - 2, n - 1


def move_object(sd, shift=(0.0, 0.0, 0.0), yaw_deg=0.0):
    """A copy of `sd` whose object (the last two triangles) is turned about the vertical axis through its centroid, then shifted."""
    v = np.asarray(sd.verts, np.float32).reshape(-1, 3, 3).copy()
    obj = v[-2:].astype(np.float64).reshape(-1, 3)
    ctr = obj.mean(axis=0)
    a = np.radians(yaw_deg)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    v[-2:] = ((obj - ctr) @ R.T + ctr + np.asarray(shift, np.float64)).reshape(2, 3, 3).astype(np.float32)
    return dataclasses.replace(sd, verts=v.reshape(-1, 9))


def object_mask(g8, sd):
    lo, hi = object_ids(sd)
    ids = g8[..., 7].view(np.uint32)
    return (ids == lo) | (ids == hi)


def interior(mask, r=2):
    """Pixels whose (2r+1)^2 neighbourhood lies in the mask."""
    m = np.pad(mask, r)
    out = np.ones_like(mask)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out &= m[dy:dy + mask.shape[0], dx:dx + mask.shape[1]]
    return out


def masked_display_rmse(a, ref, mask):
    d = np.clip(a[..., :3].astype(np.float64), 0, 1) - np.clip(ref[..., :3].astype(np.float64), 0, 1)
    return float(np.sqrt(np.mean(d[mask] ** 2)))


QUALITY_STEP = (0.0, 0.0, 0.06)  # the object comes 0.06 closer per frame: more than tau_p times its distance (3.4 * 2^-7 = 0.027)


def quality_scenes(P, w, h, frames=8):
    """The object leans back by 50 degrees, so that the ceiling light shines on the face the camera sees (upright, the light is behind
    its plane and the face shows indirect light only: nearly black, and nothing to accumulate)."""
    sd = with_object(P, P.make_scene(P.native.PT_SCENE_CORNELL, 0, 3, w, h), centre=(0.05, -0.3, 0.0), tilt_deg=0.0, lean_deg=50.0)
    return [move_object(sd, tuple(k * s for s in QUALITY_STEP)) for k in range(frames)]


def device_quality(P, r, w, h, frames=8, ref_spp=4096):
    """`frames` 1-spp frames of Cornell with the object moving towards a still camera, each followed by a DenoiseTemporal with the
    default filter, once flagged and once not; errors of the last filtered image over the object's pixels against a ref_spp frame of
    the last geometry. Returns {"display": (unflagged, flagged), "accumulated": the same of the accumulated images before the filter,
    "pixels": object pixels, "moved": stats.reserved[0] of the last call}."""
    scenes = quality_scenes(P, w, h, frames)
    out = {}
    for motion in (False, True):
        r.SetScene(scenes[0], 0)
        for k, sd in enumerate(scenes):
            if k:
                r.UpdateGeometry(verts=sd.verts)
            r.Params = P.make_params(w, h, spp=1, max_depth=8, seed=2000 + k)
            r.Render(0.0)
            st = r.DenoiseTemporal(reset=k == 0, motion=motion)
        out[motion] = (r.ReadDenoised(), st.reserved[0], r.ReadTemporal())
    mask = object_mask(r.ReadGuides(), scenes[-1])
    r.Params = P.make_params(w, h, spp=ref_spp, max_depth=8, seed=99, streams=8)
    r.Render(0.0)
    ref = r.ReadFramebuffer()
    return {"display": (masked_display_rmse(out[False][0], ref, mask), masked_display_rmse(out[True][0], ref, mask)),
            "accumulated": (masked_display_rmse(out[False][2], ref, mask), masked_display_rmse(out[True][2], ref, mask)),
            "pixels": int(mask.sum()), "moved": int(out[True][1])}


def oracle_quality(P, pto, dc, mr, w=96, h=72, frames=8, ref_spp=2048):
    """The same experiment with the checkers on the oracle's frames."""
    scenes = quality_scenes(P, w, h, frames)
    hist = {False: None, True: None}
    for k, sd in enumerate(scenes):
        scene = pto.Scene(sd)
        frame, _ = pto.render(scene, P.make_params(w, h, spp=1, max_depth=8, seed=2000 + k))
        g = dc.guides(pto, scene, w, h)
        res = {}
        for motion in (False, True):
            res[motion] = mr.accumulate(frame, g, sd.cam, sd.verts, sd.spheres, hist[motion], mr.params(flags=mr.MOTION if motion else 0))
            hist[motion] = res[motion].history
    ref, _ = pto.render(scene, P.make_params(w, h, spp=ref_spp, max_depth=8, seed=99, streams=8))
    mask = object_mask(g, scenes[-1])
    plain, flagged = (dc.filter(res[m].image, g) for m in (False, True))
    return {"display": (masked_display_rmse(plain, ref, mask), masked_display_rmse(flagged, ref, mask)),
            "accumulated": (masked_display_rmse(res[False].image, ref, mask), masked_display_rmse(res[True].image, ref, mask)),
            "pixels": int(mask.sum()), "moved": res[True].moved}
