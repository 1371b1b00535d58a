"""ctypes binding of tests/sphere_light_ref/libsphere_light_ref.so — the scalar restatement of docs/SPEC.md §7.1 (sphere lights, with the §5
loop, the §7 light sample and the §11 environment around it) that the sphere-light tests check the product against — and the scenes those
tests share. A frame through a lens takes tests/lens_ref's own ray rule. Test infrastructure only, like oracle/pto.py."""
import ctypes as C
import dataclasses

import numpy as np

import lens_checker as lc
import ref_lib

NEE, SPHERES, HITS_WEIGHT_1, AREA_PDF, SWAP_PMF, NO_PSEL, NAIVE_OMC, LAMP_BLOCKS = 1, 2, 4, 8, 16, 32, 64, 128
FLAGGED = NEE | SPHERES


class sl_stats(C.Structure):
    _fields_ = [("ext_rays", C.c_uint64), ("shadow_rays", C.c_uint64), ("paths", C.c_uint64), ("n_lights", C.c_uint64),
                ("n_sphere_lights", C.c_uint64), ("lit", C.c_uint32), ("pad", C.c_uint32)]


class sl_lens(C.Structure):
    _fields_ = [("radius", C.c_float), ("focus_distance", C.c_float)]


_f3, _f8 = C.c_float * 3, C.c_float * 8
SYMBOLS = {
    "sl_cone": (C.c_int, [_f3, C.c_float, _f3, C.c_float, C.c_float, C.c_uint32, _f8]),
    "sl_render": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(sl_lens), C.c_void_p, C.c_uint32, C.c_int, C.c_void_p,
                            C.c_void_p, C.POINTER(sl_stats)]),
}


def build():
    return ref_lib.load("sphere_light_ref", "libsphere_light_ref.so", SYMBOLS)


def cone(c, r, o, u1, u2, flags=0):
    """§7.1 in the checker's float32 for a sphere (c, r) seen from o: dict(omc, pdf, thit, wl, cosm, cos_axis), or None when o is on or
    inside the sphere."""
    out = _f8()
    if not build().sl_cone(_f3(*[float(x) for x in c]), float(r), _f3(*[float(x) for x in o]), float(u1), float(u2), flags, out):
        return None
    v = np.array(out[:], np.float32)
    return dict(omc=v[0], pdf=v[1], thit=v[2], wl=v[3:6], cosm=v[6], cos_axis=v[7])


def render(pto, scene, params, env=None, lens=None, flags=FLAGGED, with_sq=False, threads=0):
    """(rgba float32 HxWx4, sl_stats, per-pixel sums of squared sample radiance HxWx3 float64 or None). `env`: n x n x 3 or None;
    lens: (radius, focus_distance) or None."""
    lib = build()
    p = pto.pto_params()
    C.memmove(C.byref(p), C.byref(params), C.sizeof(pto.pto_params))
    out = np.zeros((p.height, p.width, 4), np.float32)
    sq = np.zeros((p.height, p.width, 3), np.float64) if with_sq else None
    e = None if env is None else np.ascontiguousarray(env, np.float32)
    ln = None if lens is None else sl_lens(*lens)
    ray = None if lens is None else C.cast(lc.build().lr_camera_ray, C.c_void_p)
    st = sl_stats()
    rc = lib.sl_render(C.addressof(scene.c), C.addressof(p), None if e is None else e.ctypes.data, 0 if e is None else e.shape[0],
                       None if ln is None else C.byref(ln), ray, flags, threads, out.ctypes.data, None if sq is None else sq.ctypes.data,
                       C.byref(st))
    if rc != 0:
        raise RuntimeError(f"sl_render failed: {rc}")
    return out, st, sq


# ----------------------------------------------------------------------------------------------------------------------------- scenes
LAMBERT, METAL, DIELECTRIC = 0, 1, 2
LAMP = ((0.0, 0.55, 0.0, 0.15), (0.0, 0.0, 0.0), (24.0, 20.0, 14.0), LAMBERT)  # centre | radius, albedo, emission, kind


def cornell(P, w, h, lamps=(LAMP,), quad=True, extra_tris=(), extra_tri_mats=(), extra_mats=()):
    """Cornell (C1), with (quad) or without its ceiling light, plus one sphere per lamp = (cxyzr, albedo, emission, kind); dielectric lamps
    have ior 1.5."""
    import nee_checker as nc
    sd = P.make_scene(P.native.PT_SCENE_CORNELL, 0, 3, w, h)
    if not quad:
        light = int(np.nonzero(sd.mats["emission"].sum(axis=1) > 0)[0][0])
        keep = sd.tri_mat != light
        sd = dataclasses.replace(sd, verts=sd.verts[keep], tri_mat=sd.tri_mat[keep])
    mats = [(kind, alb, emi, 0.0, 1.5 if kind == DIELECTRIC else 1.0) for _, alb, emi, kind in lamps] + list(extra_mats)
    return nc._with(P, sd, extra_tris, [len(lamps) + m for m in extra_tri_mats], spheres=[l[0] for l in lamps], sph_mats=list(range(len(lamps))),
                    mats=mats)


def scene(P, name, w, h):
    """The scenes of the statistical and the bit-identity tests."""
    if name == "lamp":            # lit only by a small sphere lamp
        return cornell(P, w, h, quad=False)
    if name == "lamp+quad":       # the ceiling quad and a lamp
        return cornell(P, w, h)
    if name == "glass-lamp":      # an emissive glass ball: seen from inside after refraction, weight-1 hits
        return cornell(P, w, h, lamps=(((0.3, -0.4, 0.1, 0.3), (1.0, 1.0, 1.0), (3.0, 2.5, 2.0), DIELECTRIC),))
    if name == "two-lamps":       # two lamps of different power (the pmf-swap control)
        return cornell(P, w, h, quad=False, lamps=(((-0.5, 0.6, -0.3, 0.08), (0.0, 0.0, 0.0), (90.0, 90.0, 90.0), LAMBERT),
                                                   ((0.4, 0.3, 0.2, 0.25), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), LAMBERT)))
    raise KeyError(name)


def lit_map(P, n=16):
    """A small lit environment map: a dim sky with a bright patch, seen through Cornell's open front."""
    return P.sun_sky_environment(n, (0.2, 0.3, 1.0), (30.0, 27.0, 22.0), 0.9, (0.3, 0.4, 0.6))


def without_sphere_emission(sd):
    """sd with the emission of every sphere's material removed (the spheres stay)."""
    mats = sd.mats.copy()
    for m in np.unique(sd.sph_mat):
        mats[int(m)]["emission"] = (0.0, 0.0, 0.0)
    return dataclasses.replace(sd, mats=mats)
