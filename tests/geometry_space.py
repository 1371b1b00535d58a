"""The geometry space of SPEC §4's closest hit, sampled: the cases that tests/test_geometry_space.py (oracle against the float64
caster) and tests/test_gpu_geometry_space.py (device against oracle and caster) run. Generated in code from the library's scene
generator; test helpers only.

One function per family; each returns a list of `Case`. A case names its coordinate magnitude `M` (the largest |coordinate| a ray
or a vertex of it has, to the power of two or the order of magnitude that matters) and the `ray_eps` a path trace of it uses:
`1e-4 * max(1, M)`, an absolute length that has to stay above a few ulps of the coordinates. The scale family is the one
exception: there every length of the scene is multiplied by 2^k, `ray_eps` with them (`1e-4 * 2^k`, as the scale-invariance tests
do), since a `ray_eps` of 1e-4 on a scene 2^-40 across would step over the whole scene.

Frames are W x H = 48 x 36, ray sets have N_RAYS rays, no scene has more than about 3000 triangles.

The domain (docs/SPEC.md §4 "Domain"), measured on the oracle, brute force and the host builder's five layouts, stepping k by 2
from ±30 outwards:
  frames    a 2^k rescale leaves the path-traced frames of test_power_of_two_scale_is_invisible_in_the_oracle bit-identical up to
            |k| = SCALE_K = 30; at SCALE_FIRST_BAD = ±32 they differ (+32: 71, 67 and 0 of 1728 pixels of the three scenes; -32: 0, 0
            and 2). What gives way first is not the closest hit but §5's triangle normal: dot(cr, cr) of cr = cross(e1, e2) is a
            fourth-order product, 2^(4k+4) for the Cornell walls, and leaves f32's normal range 2^-126 .. 2^128. No margin inside
            the step of 2.
  hits      the closest hit alone holds further: the glass Cornell id image is unchanged up to k = +42 and down to k = -48 and
            first differs at HIT_FIRST_BAD = (-50, +44) (16 of 1728 rays; the third-order products dot(e2, cross(tv, e1)) leave
            the range). HIT_K = 40 is what the cases use: a margin of one step above, four below.
  spheres   see ray_caster64.K_S.
"""
from dataclasses import dataclass, field, replace

import numpy as np

import adversarial_scenes as S
import ray_caster64 as rc
from float64_support import ALLOWED
from trace_support import ray_sets

W, H = 48, 36
N_RAYS = 400
SCALE_K = 30                 # the envelope: the largest |k| at which a 2^k rescale leaves ids and frames unchanged (see above)
SCALE_FIRST_BAD = (-32, 32)  # the first exponents, in steps of 2, at which a frame changes
HIT_K = 40                   # the closest hit alone: ids unchanged at least to here (measured: +42, -48)
HIT_FIRST_BAD = (-50, 44)    # the first exponents at which the id image changes
OFFSETS = [(1000.25, -333.5, 77.125), (4097.0, 4097.0, 4097.0), (65537.0, 3.0, -65537.0)]
FAR_OFFSET = (1e6, 1e6, 1e6)  # the f32 grid is 1/16 of a unit there
NEEDLE_THICKNESS = [1e-2, 1e-4, 1e-6]
CAMERA_DISTANCES = [100, 300, 1000, 3000]
SPHERE_RADII = [30, 100, 300, 1000, 3000]  # distance of the far sphere, in radii
SPHERE_R = 0.5


@dataclass
class Case:
    name: str
    family: str
    sd: object
    M: float
    ray_eps: float = None
    in_domain: bool = True
    rays: tuple = None           # (o, d) float32 to use instead of the camera rays of the W x H frame (far_sphere)
    degenerate: np.ndarray = field(default_factory=lambda: np.zeros(0, np.uint64))  # ids that may never be hit
    sphere_band: bool = False    # classify with the scaled sphere band (ray_caster64.K_S)

    def __post_init__(self):
        if self.ray_eps is None:
            self.ray_eps = 1e-4 * max(1.0, self.M)


def _P():
    return S._pkg()


def glass():
    P = _P()
    return P.make_scene(P.native.PT_SCENE_CORNELL_GLASS, 0, 5, W, H)


def tess(detail=2000):
    P = _P()
    return P.make_scene(P.native.PT_SCENE_CORNELL_TESS, detail, 5, W, H)


def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def translated(sd, offset):
    """The scene and its camera moved by `offset`: the sums are taken in float64 and rounded to f32 once."""
    out = S._clone(sd)
    off = np.asarray(offset, np.float64)
    out.verts = _f32(sd.verts.reshape(-1, 3, 3).astype(np.float64) + off).reshape(-1, 9)
    sph = sd.spheres.astype(np.float64).reshape(-1, 4).copy()
    sph[:, :3] += off
    out.spheres = _f32(sph)
    for i in range(3):
        out.cam.origin[i] = float(np.float32(sd.cam.origin[i] + off[i]))
    return out


def stretched(sd, factor):
    """x times `factor` (a power of two), vertices and camera origin. A sphere cannot be stretched: the spheres are dropped.
    A factor below 1 also narrows the camera (`right` times the factor), which would otherwise look past the sliver."""
    out = S._clone(sd)
    v = sd.verts.reshape(-1, 3, 3).copy()
    v[..., 0] *= np.float32(factor)
    out.verts = v.reshape(-1, 9)
    out.spheres, out.sph_mat = sd.spheres[:0].copy(), sd.sph_mat[:0].copy()
    out.cam.origin[0] = sd.cam.origin[0] * factor
    if factor < 1:
        for i in range(3):
            out.cam.right[i] = sd.cam.right[i] * factor
    return out


def with_triangles(sd, extra, seed):
    """`extra` (K, 9) triangles mixed into the scene's own, ids interleaved by a fixed permutation; each takes the material of a
    triangle of the scene. Returns (scene, ids of the extra triangles)."""
    rng = np.random.default_rng(seed)
    out = S._clone(sd)
    n0, k = len(sd.tri_mat), len(extra)
    verts = np.concatenate([sd.verts.reshape(-1, 9), np.asarray(extra, np.float32).reshape(-1, 9)])
    mat = np.concatenate([sd.tri_mat, sd.tri_mat[rng.integers(0, n0, k)]])
    perm = rng.permutation(n0 + k)
    out.verts, out.tri_mat = verts[perm].copy(), mat[perm].astype(np.uint32)
    return out, np.nonzero(perm >= n0)[0].astype(np.uint64)


def translate():
    out = []
    for base, sd in (("glass", glass()), ("tess", tess())):
        for i, off in enumerate(OFFSETS + [FAR_OFFSET]):
            out.append(Case(f"translate_{base}_{i}", "translate", translated(sd, off), float(np.abs(off).max())))
    return out


def scale(exponents=(-HIT_K, HIT_K)):
    out = []
    for base, sd in (("glass", glass()), ("tess", tess())):
        for k in exponents:
            out.append(Case(f"scale_{base}_{k:+d}", "scale", S.scaled(sd, k), 2.0 ** k, ray_eps=1e-4 * 2.0 ** k,
                            in_domain=abs(k) <= HIT_K))
    return out


def out_of_domain():
    """The first exponents outside the closest hit's envelope: the answer is wrong there, but specified, and the device gives the
    same one."""
    return scale(HIT_FIRST_BAD)


def needle_triangles(thickness, n=400, length=1.5, seed=21):
    """`n` triangles `length` long and `thickness` wide at random places and directions inside [-1, 1]^3 (they may poke out)."""
    rng = np.random.default_rng(seed)
    mid = rng.uniform(-0.7, 0.7, (n, 3))
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    side = np.cross(axis, rng.normal(size=(n, 3)))
    side /= np.linalg.norm(side, axis=1, keepdims=True)
    a = mid - 0.5 * length * axis
    return _f32(np.concatenate([a - 0.5 * thickness * side, a + 0.5 * thickness * side, mid + 0.5 * length * axis], axis=1))


def needles():
    out = []
    for th in NEEDLE_THICKNESS:
        sd, _ = with_triangles(tess(), needle_triangles(th), 22)
        out.append(Case(f"needles_{th:g}", "needles", sd, 1.0))
    return out


def needle_placement(sd, thickness=1e-4, n=400, seed=24):
    """The scene's vertices with `n` of its triangles (a fixed choice) moved into needles: what a refit of the committed box gets."""
    rng = np.random.default_rng(seed)
    v = sd.verts.reshape(-1, 9).copy()
    v[rng.choice(len(v), n, replace=False)] = needle_triangles(thickness, n)
    return v


def refit_cases():
    """(the tessellated box, pseudo cases of it moved) for a refit: the box carried to the translate and corridor placements and with
    400 of its triangles drawn out into needles. Vertex count and spheres' count stay the committed ones (the corridor keeps the box's
    spheres where they are)."""
    base = tess()
    out = []
    for name in ("translate_tess_0", "translate_tess_1", "translate_tess_2", "translate_tess_3", "corridor_x4096", "corridor_x2^-12"):
        c = cases()[name]
        sd = replace(c.sd, spheres=c.sd.spheres if len(c.sd.spheres) else base.spheres, sph_mat=base.sph_mat)
        out.append(Case("refit_" + name, c.family, sd, c.M))
    out.append(Case("refit_needles", "needles", replace(base, verts=needle_placement(base)), 1.0))
    return base, out


def degenerate():
    """50 each of repeated-vertex, collinear (the midpoint as middle vertex) and single-point triangles mixed into the tessellated
    box. Vertices and half-lengths are multiples of 2^-10, so a ± half is exact in f32 and a is the midpoint exactly; all three kinds
    have cross(e1, e2) == 0 exactly in float64."""
    rng = np.random.default_rng(31)
    a = (rng.integers(-920, 921, (150, 3)) / 1024.0).astype(np.float32)
    half = (rng.integers(1, 52, (150, 3)) * rng.choice([-1, 1], (150, 3)) / 1024.0).astype(np.float32)
    tri = np.empty((150, 3, 3), np.float32)
    tri[:50] = np.stack([a[:50], a[:50], a[:50] + 2 * half[:50]], axis=1)  # a repeated vertex
    tri[50:100] = np.stack([a[50:100] - half[50:100], a[50:100], a[50:100] + half[50:100]], axis=1)  # collinear
    tri[100:] = np.stack([a[100:], a[100:], a[100:]], axis=1)            # a point
    v = tri.astype(np.float64)
    assert (np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]) == 0).all()
    assert ((v[:50, 0] == v[:50, 1]).all(axis=1) & (v[:50, 0] != v[:50, 2]).any(axis=1)).all()
    assert ((v[50:100, 0] + v[50:100, 2] == 2 * v[50:100, 1]).all(axis=1) & (v[50:100, 0] != v[50:100, 2]).all(axis=1)).all()
    sd, ids = with_triangles(tess(), tri.reshape(-1, 9), 32)
    return [Case("degenerate", "degenerate", sd, 1.0, degenerate=ids)]


def corridor():
    return [Case("corridor_x4096", "corridor", stretched(tess(), 4096.0), 4096.0),
            Case("corridor_x2^-12", "corridor", stretched(tess(), 2.0 ** -12), 1.0)]


def flat():
    """Every triangle in the plane z = -0.5 (the root box has no extent along z), the Cornell camera in front of it: a 20 x 20 grid
    of quads, and a strip of 300 triangles side by side whose centroids all lie on the line y = 0."""
    base = glass()
    z = -0.5
    g = np.linspace(-1.0, 1.0, 21)
    tri = []
    for i in range(20):
        for j in range(20):
            x0, x1, y0, y1 = g[i], g[i + 1], g[j], g[j + 1]
            tri += [[x0, y0, z, x1, y0, z, x1, y1, z], [x0, y0, z, x1, y1, z, x0, y1, z]]
    xs = np.linspace(-1.0, 1.0, 300)
    strip = [[x - 0.003, -0.3, z, x + 0.003, -0.3, z, x, 0.6, z] for x in xs]  # 0.006 wide, 0.0067 apart
    out = []
    for name, t in (("flat_grid", tri), ("flat_line", strip)):
        sd = S._clone(base)
        sd.verts = _f32(t)
        sd.tri_mat = (np.arange(len(t)) % 4).astype(np.uint32)  # the walls' materials of the glass box
        sd.spheres, sd.sph_mat = base.spheres[:0].copy(), base.sph_mat[:0].copy()
        out.append(Case(name, "flat", sd, 1.0))
    return out


def mixed():
    """A 2^-12 copy of the tessellated box (1400 triangles asked for, each) inside the full one, the camera in the small copy."""
    big = tess(1400)
    small = S.scaled(big, -12)
    sd = S._clone(small)  # the small copy's camera
    sd.verts = np.concatenate([big.verts, small.verts])
    sd.tri_mat = np.concatenate([big.tri_mat, small.tri_mat])
    sd.spheres = np.concatenate([big.spheres, small.spheres])
    sd.sph_mat = np.concatenate([big.sph_mat, small.sph_mat])
    return [Case("mixed_2^-12", "mixed", sd, 1.0)]


def far_camera():
    """The glass box from `dist` units further back with a telephoto camera (scale, cx, cy times 3 / (dist + 3)), with its spheres
    (the scaled sphere band applies) and without. The spheres have radii 0.2 to 0.35: from 1000 units they are 3000 to 5000 radii
    away and from 3000 units 8500 to 15000, where the scaled band is several r² wide and excuses any disagreement that involves a
    sphere. There the classification is void for such pixels; what carries weight is the triangles-only variant and the bit
    comparison of the device with the oracle."""
    out = []
    for dist in CAMERA_DISTANCES:
        for keep in (True, False):
            sd = S._clone(glass())
            f = np.float32(3.0 / (dist + 3.0))
            sd.cam.origin[2] = sd.cam.origin[2] + float(dist)
            sd.cam.scale, sd.cam.cx, sd.cam.cy = float(sd.cam.scale * f), float(sd.cam.cx * f), float(sd.cam.cy * f)
            if not keep:
                sd.spheres, sd.sph_mat = sd.spheres[:0].copy(), sd.sph_mat[:0].copy()
            out.append(Case(f"far_camera_{dist}_{'spheres' if keep else 'triangles'}", "far_camera", sd, float(dist), sphere_band=keep))
    return out


def far_sphere(view=(0.0, 0.0, -1.0), tag="", ends=True):
    """One sphere of radius 0.5 at 30 .. 3000 radii from the origin, no triangles. The rays are a W x H fan from the origin to a
    3r x 3r square around the centre (across `view`), built in float64 and rounded to f32; about a third of them hit. `ends`: the
    grid spans the square edge to edge (else it takes the W x H cell centres)."""
    base = glass()
    view = np.asarray(view, np.float64)
    view = view / np.linalg.norm(view)
    right = np.cross(view, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, view)
    if ends:
        gx, gy = np.linspace(-1.5, 1.5, W) * SPHERE_R, np.linspace(-1.5, 1.5, H) * SPHERE_R
    else:
        gx, gy = ((np.arange(W) + 0.5) / W - 0.5) * 3 * SPHERE_R, ((np.arange(H) + 0.5) / H - 0.5) * 3 * SPHERE_R
    out = []
    for n in SPHERE_RADII:
        centre = _f32(view * n * SPHERE_R)
        target = centre.astype(np.float64) + gx[None, :, None] * right + gy[:, None, None] * up
        d = target.reshape(-1, 3)
        d = _f32(d / np.linalg.norm(d, axis=1, keepdims=True))
        sd = S._clone(base)
        sd.verts, sd.tri_mat = np.zeros((0, 9), np.float32), np.zeros(0, np.uint32)
        sd.spheres, sd.sph_mat = np.array([[*centre, SPHERE_R]], np.float32), base.sph_mat[:1].copy()
        for i in range(3):
            sd.cam.origin[i] = 0.0
        out.append(Case(f"far_sphere{tag}_{n}", "far_sphere", sd, n * SPHERE_R, rays=(np.zeros_like(d), d), sphere_band=True))
    return out


def silhouette_ring(case, rel, n=N_RAYS):
    """`n` rays from the origin to a ring of radius rel · r around a far_sphere case's centre, across the line of sight."""
    c = case.sd.spheres[0, :3].astype(np.float64)
    view = c / np.linalg.norm(c)
    right = np.cross(view, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, view)
    a = (np.arange(n) + 0.5) * (2 * np.pi / n)
    p = c + rel * SPHERE_R * (np.cos(a)[:, None] * right + np.sin(a)[:, None] * up)
    d = _f32(p / np.linalg.norm(p, axis=1, keepdims=True))
    return np.zeros_like(d), d


def far_sphere_oblique():
    """The same spheres off every axis, (0.3, -0.2, -1), under a fan through the cell centres: every component of oc rounds, which an
    axis-aligned oc spares §4's discriminant. Here disagreements begin at 300 radii (7 of 1728), as (|oc|/r)² · 2^-24 predicts."""
    return far_sphere((0.3, -0.2, -1.0), "_oblique", ends=False)


FAMILIES = [translate, scale, needles, degenerate, corridor, flat, mixed, far_camera, far_sphere, far_sphere_oblique]


def in_domain_cases():
    return [c for fam in FAMILIES for c in fam()]


def all_cases():
    return in_domain_cases() + out_of_domain()


def find(name):
    return next(c for c in all_cases() if c.name == name)


def case_rays(pto, case):
    """The rays a case is traced with: its own, or the camera rays (SPEC §3, key 0, jittered as the generator's cameras are) of the W x H frame."""
    if case.rays is not None:
        return case.rays
    return rc.camera_rays(pto, case.sd.cam, W, H)


# ---- what every implementation's ids have to pass on a case (the oracle in tests/test_geometry_space.py, the device in
# tests/test_gpu_geometry_space.py)
RAY_SET_FAMILIES = ("translate", "needles", "corridor")
ORIGIN_CAP = 0.5 * 400 / 2362  # half the share of needles among a needle scene's triangles: 8.5 % (3.2 % seen)
COUNTS = {}  # context -> class sizes of every check_case call, for whoever runs the tests from a script and wants the figures
_CASES = {}


def cases():
    """name -> Case, built once for the session and never changed."""
    if not _CASES:
        _CASES.update((c.name, c) for c in all_cases())
    return _CASES


CASE_NAMES = [c for fam in ("translate_glass", "translate_tess") for c in (f"{fam}_{i}" for i in range(4))] + \
    ["scale_glass_-40", "scale_glass_+40", "scale_tess_-40", "scale_tess_+40", "needles_0.01", "needles_0.0001", "needles_1e-06",
     "degenerate", "corridor_x4096", "corridor_x2^-12", "flat_grid", "flat_line", "mixed_2^-12"] + \
    [f"far_camera_{d}_{k}" for d in CAMERA_DISTANCES for k in ("spheres", "triangles")] + \
    [f"far_sphere{t}_{n}" for t in ("", "_oblique") for n in SPHERE_RADII]

# the cases whose rays are made on surfaces: the full path trace of tests/test_gpu_geometry_space.py and the gathers of
# tests/test_gpu_gather_space.py
PATH_TRACE = ["translate_glass_0", "translate_tess_0", "translate_glass_2", "translate_tess_2", "needles_0.0001", "degenerate",
              "corridor_x4096", "corridor_x2^-12", "flat_grid", "flat_line", "scale_glass_-40", "scale_glass_+40", "scale_tess_-40",
              "scale_tess_+40"]


def counts(c):
    return {k: len(v) for k, v in c.items() if k not in ("want", "sphere_ratio")}


def check_case(case, rs, o, d, ids, cast, ctx):
    """The assertions every f32 implementation's ids have to pass on a case's ray set `rs`; returns the classes' sizes.

    wrong == 0. in_plane == 0, except that rays along an axis (the zero-component set) of a translated scene may run in the plane of
    an axis-aligned wall: at most 1 %. edge + coincident <= ALLOWED of the rays; for the zero-component rays at the offset of 65537
    the cap is 2.5 %: f32's grid is 2^-8 there, so origins and walls snap to it and 1.75 % of such rays graze an edge in float64. On a
    case with far spheres the cap holds for what the unscaled bands explain; what only the scaled sphere band explains is not capped
    (its size follows from the distance: 8.6 % of the frame at 1000 units), but none may lie outside it. No degenerate triangle is hit.
    At the offset of 1e6 every coordinate lies on f32's grid of 1/16, 33 values across the box. The three extra ray sets start on that
    grid: an axis ray lies in a wall's plane when its origin has the wall's coordinate (2 of 33 values, the end ones at half weight)
    and no component along the wall's normal (5 of the 9 directions), 3 · 1/32 · 5/9 = 5.2 % at most (3 % seen); and it runs along a
    mesh line of the tessellated box, where float64 cannot say what f32 should do, far more often than a ray of a continuum does.
    Their edge + coincident cap is 5 % (3.5 % seen on the axis rays, 1.25 % on the incoherent ones), as 2.5 % is at 65537.
    On the needle scenes a ray of the on-surface set may start on an oblique triangle, a rounded point a few ulps off its plane;
    whether that triangle is hit at once is the class `origin` of ray_caster64.classify, which holds the rest of the answer to the
    caster. The floor is 16 ulps of the origin's largest coordinate (3 ulps off the plane at a cosine of 0.2). Such rays are at most
    half of those that start on a needle (float64 puts the start in front of the triangle for half of them), needles being 400 of
    the scene's triangles: ORIGIN_CAP of the set."""
    sd = case.sd
    floor = None
    if rs == "on_surface" and case.family == "needles":
        floor = 16 * np.spacing(np.abs(o).max(axis=1)).astype(np.float64)
    c = rc.classify(sd.verts, sd.spheres, o, d, ids, cast, sphere_band=case.sphere_band, t_floor=floor)
    n = counts(c)
    COUNTS[ctx] = n
    assert n["wrong"] == 0, (ctx, n, c["wrong"][:10], ids[c["wrong"][:10]], c["want"][c["wrong"][:10]])
    assert n["origin"] <= ORIGIN_CAP * len(o), (ctx, n)
    axis_rays = rs == "zero_components" and case.family == "translate"
    on_grid = case.M == 1e6 and rs != "camera"
    assert n["in_plane"] <= ((0.052 if on_grid else 0.01) * len(o) if axis_rays else 0), (ctx, n)
    capped = counts(rc.classify(sd.verts, sd.spheres, o, d, ids, cast, t_floor=floor)) if case.sphere_band else n
    cap = 0.05 if on_grid else 0.025 if axis_rays and case.M == 65537.0 else ALLOWED
    assert capped["edge"] + capped["coincident"] <= cap * len(o), (ctx, capped)
    assert not np.isin(ids, case.degenerate).any(), ctx
    if case.family == "far_sphere" and case.name.rsplit("_", 1)[0] == "far_sphere" and case.M <= 300 * SPHERE_R:
        assert n["agree"] == len(o), (ctx, n)  # on the axis, up to 300 radii: no disagreement at all
    return n


def case_ray_sets(pto, case):
    sets = [("camera",) + tuple(case_rays(pto, case))]
    if case.family in RAY_SET_FAMILIES:
        sets += [s for s in ray_sets(pto, case.sd, n=N_RAYS) if s[0] != "camera"]
    return sets
