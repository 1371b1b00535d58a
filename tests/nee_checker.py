"""ctypes binding of tests/nee_ref/libnee_ref.so — the scalar restatement of docs/SPEC.md §7 (next-event estimation) that the NEE tests
check the device against. Test infrastructure only, like oracle/pto.py; `build()` runs its Makefile."""
import ctypes as C

import numpy as np

import ref_lib

NEE, NO_MIS, NO_COSL, SWAP_PMF = 1, 2, 4, 8


class nr_stats(C.Structure):
    _fields_ = [("ext_rays", C.c_uint64), ("shadow_rays", C.c_uint64), ("paths", C.c_uint64), ("n_lights", C.c_uint64)]


# name -> (restype, argtypes): the entry points of nee_ref.c
SYMBOLS = {
    "nr_render": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(nr_stats)]),
}


def build():
    """The checker, made (incrementally) and loaded on the first call of a process."""
    return ref_lib.load("nee_ref", "libnee_ref.so", SYMBOLS)


def render(pto, scene, params, flags=NEE, with_sq=False, threads=0):
    """(rgba float32 HxWx4, nr_stats, per-pixel sums of squared sample radiance HxWx3 float64 or None). `scene`: a pto.Scene (brute
    force or with a blob: the picture is the same); `params`: any ctypes struct with the pt_render_params layout."""
    lib = build()
    p = pto.pto_params()
    C.memmove(C.byref(p), C.byref(params), C.sizeof(pto.pto_params))
    out = np.zeros((p.height, p.width, 4), np.float32)
    sq = np.zeros((p.height, p.width, 3), np.float64) if with_sq else None
    st = nr_stats()
    rc = lib.nr_render(C.addressof(scene.c), C.addressof(p), flags, threads, out.ctypes.data,
                       None if sq is None else sq.ctypes.data, C.byref(st))
    if rc != 0:
        raise RuntimeError(f"nr_render failed: {rc}")
    return out, st, sq


# ---------------------------------------------------------------------------------------------------------------- scenes of the NEE tests
def _with(P, sd, tris=(), tri_mats=(), spheres=(), sph_mats=(), mats=()):
    """sd plus extra triangles (9 floats each), spheres (4 floats each) and materials (tuples kind, albedo3, emission3, roughness, ior);
    material ids in tri_mats / sph_mats index the extra materials."""
    import dataclasses
    nm = len(sd.mats)
    extra = np.zeros(len(mats), sd.mats.dtype)
    for i, (kind, alb, emi, rough, ior) in enumerate(mats):
        extra[i]["kind"], extra[i]["albedo"], extra[i]["emission"], extra[i]["roughness"], extra[i]["ior"] = kind, alb, emi, rough, ior
    return dataclasses.replace(
        sd, verts=np.concatenate([sd.verts, np.asarray(tris, np.float32).reshape(-1, 9)]),
        tri_mat=np.concatenate([sd.tri_mat, np.asarray(tri_mats, np.uint32) + nm]),
        spheres=np.concatenate([sd.spheres, np.asarray(spheres, np.float32).reshape(-1, 4)]),
        sph_mat=np.concatenate([sd.sph_mat, np.asarray(sph_mats, np.uint32) + nm]),
        mats=np.concatenate([sd.mats, extra]))


def many_lights_scene(P, w, h, seed=5):
    """Cornell (C1) plus 24 emissive triangles of different sizes and emissions on the walls, an emissive rough-metal triangle, a
    zero-area emissive triangle (not a light) and an emissive sphere (found by hits only)."""
    sd = P.make_scene(P.native.PT_SCENE_CORNELL, 0, 3, w, h)
    rng = np.random.default_rng(seed)
    mats = [(0, (0.5, 0.5, 0.5), (4.0, 2.0, 1.0), 0.0, 1.0), (0, (0.2, 0.2, 0.2), (0.5, 0.5, 6.0), 0.0, 1.0),
            (0, (0.0, 0.0, 0.0), (20.0, 20.0, 20.0), 0.0, 1.0), (1, (0.9, 0.9, 0.9), (1.0, 3.0, 1.0), 0.3, 1.0),
            (0, (0.7, 0.7, 0.7), (2.0, 6.0, 2.0), 0.0, 1.0)]
    tris, tm = [], []
    for i in range(24):
        wall = i % 3  # back (z = -0.999), left (x = -0.999), right (x = 0.999)
        c = rng.uniform(-0.8, 0.8, 2)
        s = rng.uniform(0.01, 0.25)
        a, b = c + rng.uniform(-s, s, 2), c + rng.uniform(-s, s, 2)
        pts = [c, a, b]
        if wall == 0:
            v = [(p[0], p[1], -0.999) for p in pts]
        elif wall == 1:
            v = [(-0.999, p[1], p[0]) for p in pts]
        else:
            v = [(0.999, p[1], p[0]) for p in pts]
        tris.append(np.ravel(v)); tm.append(i % 3)
    tris.append([0.3, -0.99, 0.2, 0.7, -0.99, 0.1, 0.5, -0.6, -0.1]); tm.append(3)   # emissive metal triangle
    tris.append([0.1, 0.5, -0.9, 0.1, 0.5, -0.9, 0.2, 0.6, -0.9]); tm.append(0)      # zero area
    return _with(P, sd, tris, tm, spheres=[(0.0, 0.2, 0.0, 0.15)], sph_mats=[4], mats=mats)


def grazing_scene(P, w, h):
    """Lights at grazing and point-blank distance from Lambert surfaces: one standing edge-on on the floor, one a hair above the floor
    facing it, one lying in the plane of the back wall a hair in front of it, and one tiny one inside the ray_eps of the floor."""
    sd = P.make_scene(P.native.PT_SCENE_CORNELL, 0, 3, w, h)
    mats = [(0, (0.5, 0.5, 0.5), (8.0, 8.0, 8.0), 0.0, 1.0)]
    tris = [[-0.5, -1.0, 0.0, 0.5, -1.0, 0.0, 0.0, -0.4, 0.0],                   # edge-on, standing on the floor
            [-0.6, -0.99999, 0.5, -0.2, -0.99999, 0.5, -0.4, -0.99999, 0.1],       # parallel to the floor, 1e-5 above it
            [0.2, -0.5, -0.99999, 0.6, -0.5, -0.99999, 0.4, -0.1, -0.99999],       # in front of the back wall
            [0.1, -0.99995, 0.6, 0.10001, -0.99995, 0.6, 0.1, -0.99995, 0.60001]]  # tiny, within ray_eps of the floor
    return _with(P, sd, tris, [0, 0, 0, 0], mats=mats)


def two_lights_scene(P, w, h):
    """Cornell with its ceiling light replaced by two lights of different size and emission (the pmf-swap control)."""
    sd = P.make_scene(P.native.PT_SCENE_CORNELL, 0, 3, w, h)
    light = int(np.nonzero(sd.mats["emission"].sum(axis=1) > 0)[0][0])
    keep = sd.tri_mat != light
    import dataclasses
    sd = dataclasses.replace(sd, verts=sd.verts[keep], tri_mat=sd.tri_mat[keep])
    mats = [(0, (0.0, 0.0, 0.0), (30.0, 30.0, 30.0), 0.0, 1.0), (0, (0.0, 0.0, 0.0), (0.5, 0.5, 0.5), 0.0, 1.0)]
    small = [-0.6, 0.998, -0.6, -0.4, 0.998, -0.6, -0.6, 0.998, -0.4]
    big = [0.0, 0.998, -0.2, 0.8, 0.998, -0.2, 0.0, 0.998, 0.6]
    return _with(P, sd, [small, big], [0, 1], mats=mats)
