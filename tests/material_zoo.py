"""A material zoo: small valid scenes that take the BSDFs of docs/SPEC.md §5 through the parts of the material space the generator
scenes (scenegen.cpp: one glass, one gold, one mirror sphere; every triangle Lambert) leave alone — rough metal at exact normal
incidence and at large and tiny roughness, dielectric triangles, total internal reflection inside flat-sided glass, ior below, at
and next to 1, black and over-unit albedos, emission on every kind, back faces, long material tables. Test helpers only.

Every scene has at most about 150 triangles and 16 spheres and is rendered at 64x48; every camera has jitter off, so which branch
a vertex reaches does not depend on sub-pixel offsets. `CONFIGS` names the (scene, camera) pairs, `CLAIMS` the branch classes of
tests/census_ref/ each pair is built to reach (the docstring of each builder lists the same names; the CPU tests hold both)."""
import itertools

import numpy as np

LAMBERT, METAL, DIELECTRIC = 0, 1, 2
W, H = 64, 48

# the grid of the issue: every value appears in some scene (test_materials.test_grid_is_covered)
ROUGHNESS = (0.0, 1e-4, 0.02, 0.15, 0.5, 1.0)
IOR = (0.5, 0.75, 1.0, 1.0001, 1.33, 1.5, 2.4, 50.0)
ALBEDO = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.0, 0.5, 0.0), (1.5, 1.2, 0.9), (1e-30, 1e-30, 1e-30))

CLASSES = ("L_front", "L_back", "M_mirror", "M_rough", "M_rough_dead", "M_rough_normal",
           "D_reflect_front", "D_reflect_back", "D_refract_front", "D_refract_back", "D_tir_front", "D_tir_back", "D_on_triangle",
           "T_black", "RR_kill", "RR_survive_clamped", "RR_survive_unclamped", "depth_cut",
           "emit_metal", "emit_dielectric", "emit_sphere", "miss")


def _pkg():
    """pathtracing_amd, imported on first use (libptrt.so exists only once the session's build fixture has run)."""
    import pathtracing_amd
    return pathtracing_amd


# ------------------------------------------------------------------------------------------------------------------------ building blocks
def mat(kind, albedo, emission=(0.0, 0.0, 0.0), roughness=0.0, ior=1.5):
    return (kind, tuple(albedo), tuple(emission), roughness, ior)


def quad(p0, eu, ev):
    """Two triangles over p0 + s*eu + t*ev, s, t in [0, 1]; geometric normal along cross(eu, ev)."""
    p0, eu, ev = (np.asarray(v, np.float64) for v in (p0, eu, ev))
    return [np.concatenate([p0, p0 + eu, p0 + eu + ev]), np.concatenate([p0, p0 + eu + ev, p0 + ev])]


def camera(origin, target=None, up=(0.0, 1.0, 0.0), fov_deg=50.0, forward=None, pinned=False):
    """A pt_camera with jitter off. `pinned`: right = up = 0, so every pixel casts the ray `forward` from `origin` (with its own
    random numbers) — whole frames at one exact incidence."""
    N = _pkg().native
    cam = N.pt_camera()
    o = np.asarray(origin, np.float64)
    f = np.asarray(forward, np.float64) if forward is not None else np.asarray(target, np.float64) - o
    f = f / np.linalg.norm(f)
    r = np.cross(f, np.asarray(up, np.float64)); r /= np.linalg.norm(r)
    u = np.cross(r, f)
    th = 0.0 if pinned else np.tan(np.radians(fov_deg) / 2)
    for k in range(3):
        cam.origin[k], cam.forward[k], cam.right[k], cam.up[k] = o[k], f[k], th * r[k], -th * u[k]
    cam.scale, cam.cx, cam.cy, cam.jitter = 2.0 / H, W / H, 1.0, 0
    return cam


def scene(tris, tri_mats, spheres, sph_mats, mats, cam, sky):
    P = _pkg()
    m = np.zeros(len(mats), P.MATERIAL_DTYPE)
    for i, (kind, alb, emi, rough, ior) in enumerate(mats):
        m[i]["kind"], m[i]["albedo"], m[i]["emission"], m[i]["roughness"], m[i]["ior"] = kind, alb, emi, rough, ior
    return P.SceneData(verts=np.asarray(tris, np.float32).reshape(-1, 9), tri_mat=np.asarray(tri_mats, np.uint32),
                       spheres=np.asarray(spheres, np.float32).reshape(-1, 4), sph_mat=np.asarray(sph_mats, np.uint32),
                       mats=m, cam=cam, sky=np.asarray(sky, np.float32))


# ------------------------------------------------------------------------------------------------------------------------------- slabs
SLAB_MATS = (
    [mat(METAL, (0.9, 0.8, 0.6), roughness=r) for r in ROUGHNESS]                                  # 0..5: the roughness grid
    + [mat(DIELECTRIC, (1.0, 1.0, 1.0), ior=i) for i in IOR]                                      # 6..13: the ior grid
    + [mat(LAMBERT, a) for a in ALBEDO]                                                           # 14..18: the albedo grid
    + [mat(METAL, (1.5, 1.2, 0.9), roughness=0.5), mat(METAL, (0.0, 0.5, 0.0), roughness=0.0),    # 19..23: odd albedos elsewhere
       mat(DIELECTRIC, (1.5, 1.2, 0.9), ior=1.5), mat(DIELECTRIC, (0.0, 0.5, 0.0), ior=1.33),
       mat(METAL, (0.0, 0.0, 0.0), roughness=0.15)])
SLAB_COLS, SLAB_ROWS = 6, 4
# pinned views: the slab each looks straight down on (metal of roughness 1, 1e-4, 0.02; glass of ior 0.5, 1, 1.0001, 50)
PINNED_SLAB = {"normal": 5, "normal_r1e4": 1, "normal_r002": 2, "normal_glass": 6, "normal_ior1": 8, "normal_ior10001": 9,
               "normal_ior50": 13}


def slab_centre(i):
    return (i % SLAB_COLS) - SLAB_COLS / 2 + 0.5, (i // SLAB_COLS) - SLAB_ROWS / 2 + 0.5


def slabs(view):
    """Axis-aligned unit quads in the plane z = 0 (normal +z), one per material of SLAB_MATS, over a Lambert floor at z = -1, under an
    emissive Lambert ceiling, between an emissive rough-metal wall and an emissive glass wall.
    view "normal": a pinned camera above slab 5 (metal, roughness 1) looking along -z: every path starts at exact normal incidence
    (lensq == 0, T1 = (1,0,0)), where roughness 1 also kills many samples. view "normal_glass": the same above slab 6 (ior 0.5).
    views "normal_r1e4", "normal_r002", "normal_ior1", "normal_ior10001", "normal_ior50": the same above the slabs of roughness
    1e-4 and 0.02 and of ior 1, 1.0001 and 50 (PINNED_SLAB): lensq == 0 and cosi == 1 where the roundings differ most.
    view "oblique": a perspective camera that sees the slabs obliquely: TIR on the front of ior < 1, every roughness.
    Classes (normal): M_rough M_rough_dead M_rough_normal L_front D_refract_back D_tir_back D_on_triangle T_black RR_kill emit_metal
    emit_dielectric miss
    Classes (normal_glass): D_reflect_front D_refract_front D_refract_back D_tir_back D_on_triangle L_front L_back M_rough T_black
    RR_kill RR_survive_clamped RR_survive_unclamped emit_metal miss
    Classes (normal_r1e4): M_rough M_rough_normal miss
    Classes (normal_r002): M_rough M_rough_normal L_front T_black miss
    Classes (normal_ior1): D_refract_front D_refract_back D_on_triangle L_front L_back RR_kill miss
    Classes (normal_ior10001): D_refract_front D_refract_back D_on_triangle L_front L_back RR_kill miss
    Classes (normal_ior50): D_reflect_front D_refract_front D_on_triangle L_front T_black miss
    Classes (oblique): L_front L_back M_mirror M_rough M_rough_dead D_reflect_front D_refract_front D_refract_back D_tir_front
    D_tir_back D_on_triangle T_black RR_kill RR_survive_clamped RR_survive_unclamped emit_metal emit_dielectric miss"""
    tris, tm = [], []
    for i in range(len(SLAB_MATS)):
        cx, cy = slab_centre(i)
        tris += quad((cx - 0.5, cy - 0.5, 0.0), (1, 0, 0), (0, 1, 0)); tm += [i, i]
    nm = len(SLAB_MATS)
    mats = list(SLAB_MATS) + [mat(LAMBERT, (0.7, 0.7, 0.7)),                                         # nm: floor
                              mat(LAMBERT, (0.0, 0.0, 0.0), emission=(6.0, 5.0, 4.0)),               # nm+1: ceiling light
                              mat(METAL, (0.8, 0.8, 0.8), emission=(0.5, 1.0, 2.0), roughness=0.5),  # nm+2: emissive metal wall
                              mat(DIELECTRIC, (1.0, 1.0, 1.0), emission=(2.0, 0.5, 0.5), ior=1.5)]   # nm+3: emissive glass wall
    tris += quad((-5, -4, -1.0), (10, 0, 0), (0, 8, 0)); tm += [nm, nm]          # floor, normal +z
    tris += quad((-2, -1.5, 5.0), (0, 3, 0), (4, 0, 0)); tm += [nm + 1, nm + 1]  # ceiling light, normal -z
    tris += quad((-4.5, -3, -1.0), (0, 0, 5), (0, 6, 0)); tm += [nm + 2, nm + 2]  # wall at x = -4.5, normal +x
    tris += quad((4.5, -3, -1.0), (0, 6, 0), (0, 0, 5)); tm += [nm + 3, nm + 3]  # wall at x = +4.5, normal -x
    if view == "oblique":
        cam = camera((-0.4, -4.6, 3.2), (0.0, -0.1, 0.0), up=(0, 0, 1), fov_deg=62)
    else:
        cx, cy = slab_centre(PINNED_SLAB[view])
        cam = camera((cx + 0.25, cy - 0.125, 2.0), forward=(0, 0, -1), up=(0, 1, 0), pinned=True)  # off the quad's diagonal
    return scene(tris, tm, [], [], mats, cam, (0.05, 0.06, 0.08))


# --------------------------------------------------------------------------------------------------------------------------- glass_box
def glass_box(view):
    """A closed cube [-1,1]^3 of dielectric triangles (ior 1.5; the top face 1.33, the +x face 2.4) around a small Lambert
    tetrahedron, a mirror sphere and a small emissive sphere, on a Lambert floor under an emissive quad.
    view "outside": a camera in front of the cube. view "inside": a camera inside the cube looking at an edge, so that the first
    vertex is a back face (front == false at vertex 0) and the walls are met beyond the critical angle: total internal reflection.
    Classes (outside): D_reflect_front D_refract_front D_refract_back D_reflect_back D_tir_back D_on_triangle L_front M_mirror
    emit_sphere RR_kill RR_survive_clamped RR_survive_unclamped miss
    Classes (inside): D_refract_back D_reflect_back D_tir_back D_on_triangle L_front M_mirror emit_sphere T_black depth_cut RR_kill
    RR_survive_clamped"""
    g15, g133, g24 = 0, 1, 2
    mats = [mat(DIELECTRIC, (1.0, 1.0, 1.0), ior=1.5), mat(DIELECTRIC, (1.0, 1.0, 1.0), ior=1.33),
            mat(DIELECTRIC, (0.95, 1.0, 0.95), ior=2.4),
            mat(LAMBERT, (0.8, 0.3, 0.2)),                                   # 3: tetrahedron
            mat(METAL, (0.95, 0.95, 0.95), roughness=0.0),                   # 4: mirror sphere
            mat(LAMBERT, (0.0, 0.0, 0.0), emission=(12.0, 10.0, 8.0)),       # 5: emissive sphere inside
            mat(LAMBERT, (0.6, 0.6, 0.6)),                                   # 6: floor
            mat(LAMBERT, (0.0, 0.0, 0.0), emission=(8.0, 8.0, 8.0))]         # 7: light quad
    tris, tm = [], []
    faces = [((-1, -1, 1), (2, 0, 0), (0, 2, 0), g15),    # +z
             ((1, -1, -1), (-2, 0, 0), (0, 2, 0), g15),   # -z
             ((1, -1, 1), (0, 0, -2), (0, 2, 0), g24),    # +x
             ((-1, -1, -1), (0, 0, 2), (0, 2, 0), g15),   # -x
             ((-1, 1, 1), (2, 0, 0), (0, 0, -2), g133),   # +y
             ((-1, -1, -1), (2, 0, 0), (0, 0, 2), g15)]   # -y
    for p0, eu, ev, m in faces:
        tris += quad(p0, eu, ev); tm += [m, m]
    a, b, c, d = (np.array(v) for v in ((-0.5, -0.6, -0.2), (-0.1, -0.6, -0.3), (-0.3, -0.6, 0.2), (-0.3, -0.2, -0.1)))
    for t in ((a, c, b), (a, b, d), (b, c, d), (c, a, d)):
        tris.append(np.concatenate(t)); tm.append(3)
    tris += quad((-4, -1.5, -4), (0, 0, 8), (8, 0, 0)); tm += [6, 6]        # floor, normal +y
    tris += quad((-1.5, 3.0, -1.5), (3, 0, 0), (0, 0, 3)); tm += [7, 7]     # light, normal -y
    spheres = [(0.45, -0.3, -0.3, 0.3), (0.1, 0.45, 0.3, 0.12)]
    if view == "outside":
        cam = camera((1.2, 1.1, 4.2), (0.0, -0.1, 0.0), fov_deg=42)
    else:
        cam = camera((-0.55, 0.3, 0.55), (1.0, -0.2, -1.0), fov_deg=80)
    return scene(tris, tm, spheres, [4, 5], mats, cam, (0.10, 0.12, 0.16))


# ------------------------------------------------------------------------------------------------------------------------------ shells
def shells(view):
    """Nested and neighbouring spheres: a glass ball (ior 1.5) with an ior 0.75 bubble inside it, an ior 1.0 ball (F = 0: it only
    ever reflects inside the float32 grazing band of SPEC §5), an ior 1.0001 ball, an ior 50 ball, a rough-metal ball and an
    emissive ball over a Lambert floor.
    view "outside": a camera that sees all of them. view "inside": a camera inside the glass ball, off its centre, between the
    bubble and the wall: the first vertex is a back face or the bubble's front (ior 0.75: TIR on the front side).
    Classes (outside): D_reflect_front D_refract_front D_refract_back D_reflect_back D_tir_front M_rough L_front emit_sphere miss
    RR_kill RR_survive_unclamped
    Classes (inside): D_refract_back D_reflect_back D_tir_back D_tir_front D_refract_front L_front emit_sphere depth_cut RR_kill
    RR_survive_clamped miss"""
    mats = [mat(DIELECTRIC, (1.0, 1.0, 1.0), ior=1.5), mat(DIELECTRIC, (1.0, 1.0, 1.0), ior=0.75),
            mat(DIELECTRIC, (1.0, 0.9, 0.9), ior=1.0), mat(DIELECTRIC, (0.9, 1.0, 0.9), ior=1.0001),
            mat(DIELECTRIC, (0.9, 0.9, 1.0), ior=50.0), mat(METAL, (0.9, 0.6, 0.3), roughness=0.15),
            mat(LAMBERT, (0.0, 0.0, 0.0), emission=(10.0, 9.0, 8.0)), mat(LAMBERT, (0.6, 0.6, 0.6))]
    spheres = [(-1.2, 0.0, 0.0, 1.0), (-1.2, 0.0, 0.0, 0.5), (1.1, -0.3, 0.0, 0.7), (0.9, 1.2, 0.0, 0.45),
               (-0.4, 1.6, 0.0, 0.45), (2.4, 0.6, -0.5, 0.5), (0.3, 3.2, 1.0, 0.6)]
    tris = quad((-6, -1.0, -6), (0, 0, 12), (12, 0, 0))
    if view == "outside":
        cam = camera((0.3, 0.9, 6.0), (0.2, 0.5, 0.0), fov_deg=50)
    else:
        cam = camera((-1.2, 0.0, 0.75), (1.0, 0.4, 0.0), fov_deg=100)
    return scene(tris, [7, 7], spheres, [0, 1, 2, 3, 4, 5, 6], mats, cam, (0.3, 0.35, 0.45))


# ----------------------------------------------------------------------------------------------------------------------------- palette
def palette_materials():
    """320 materials: the whole grid (5 Lambert, 30 metal, 40 dielectric) four times over, then 20 emissive ones of every kind."""
    grid = ([mat(LAMBERT, a) for a in ALBEDO] + [mat(METAL, a, roughness=r) for r, a in itertools.product(ROUGHNESS, ALBEDO)]
            + [mat(DIELECTRIC, a, ior=i) for i, a in itertools.product(IOR, ALBEDO)])
    mats = grid * 4
    for j in range(20):
        k = (LAMBERT, METAL, DIELECTRIC)[j % 3]
        e = (1.0 + j % 4, 0.5 * (1 + j % 3), 2.0 - 0.25 * (j % 5))
        mats.append(mat(k, ALBEDO[1 + j % 3], emission=e, roughness=ROUGHNESS[j % 6], ior=IOR[j % 8]))
    return mats


def palette(view="front"):
    """An open soup of 120 triangles and 16 spheres over a table of 320 materials drawn from the whole grid; every primitive has its
    own material id, ids up to the last of the table are in use, and nine triangles (Lambert, metal and dielectric ones) and one
    sphere emit. Back faces of Lambert triangles are hit, the light set of SPEC §7 holds lights of every kind, and the denoiser's
    g1 holds albedos of every kind.
    Classes (front): L_front L_back M_mirror M_rough M_rough_dead D_reflect_front D_reflect_back D_refract_front D_refract_back
    D_tir_front D_tir_back D_on_triangle T_black RR_kill RR_survive_clamped RR_survive_unclamped emit_metal emit_dielectric
    emit_sphere miss"""
    rng = np.random.default_rng(20240)
    mats = palette_materials()
    nm, nt, ns = len(mats), 120, 16
    ids = rng.permutation(nm - 20)[: nt + ns - 10]
    ids = np.concatenate([ids, np.arange(nm - 10, nm)])  # the last ten (emissive, every kind) are all in use
    tris = []
    for _ in range(nt):
        c = rng.uniform(-2.2, 2.2, 3) * (1.0, 0.8, 0.6)
        tris.append(np.concatenate([c + rng.uniform(-0.7, 0.7, 3) for _ in range(3)]))
    tri_mats = np.concatenate([ids[: nt - 9], ids[-10:-1]])  # nine emissive triangles, every kind among them
    sph_mats = np.concatenate([ids[nt - 9: nt - 9 + ns - 1], ids[-1:]])  # one emissive sphere
    spheres = [tuple(rng.uniform(-2.0, 2.0, 3) * (1.0, 0.8, 0.5)) + (rng.uniform(0.15, 0.4),) for _ in range(ns)]
    cam = camera((0.2, 0.3, 5.5), (0.0, 0.0, 0.0), fov_deg=48)
    return scene(tris, tri_mats, spheres, sph_mats, mats, cam, (0.4, 0.45, 0.5))


# ------------------------------------------------------------------------------------------------------------------- configurations
BUILDERS = {"slabs": slabs, "glass_box": glass_box, "shells": shells, "palette": palette}
CONFIGS = [("slabs", "normal"), ("slabs", "normal_glass"), ("slabs", "normal_r1e4"), ("slabs", "normal_r002"), ("slabs", "normal_ior1"),
           ("slabs", "normal_ior10001"), ("slabs", "normal_ior50"), ("slabs", "oblique"), ("glass_box", "outside"), ("glass_box", "inside"),
           ("shells", "outside"), ("shells", "inside"), ("palette", "front")]


def build(name, view):
    return BUILDERS[name](view)


def _claims():
    out = {}
    for name, fn in BUILDERS.items():
        for piece in fn.__doc__.split("Classes (")[1:]:
            view, text = piece.split("):", 1)
            assert all(w in CLASSES for w in text.split()), (name, view, text)
            out[(name, view)] = tuple(text.split())
    return out


CLAIMS = _claims()  # (scene, view) -> the classes its docstring says it reaches


def parity_params(P, flags=0):
    """The parameters of the device parity frames (tests/test_gpu_materials.py) and of the census."""
    return P.make_params(W, H, spp=4, max_depth=12, rr_start=3, streams=2, flags=flags)


EDGE_SCENES = [("slabs", "oblique"), ("slabs", "normal"), ("glass_box", "outside"), ("glass_box", "inside")]
EDGE_PARAMS = {  # depth and roulette edges on slabs and glass_box
    "depth1": dict(spp=4, max_depth=1, rr_start=3, streams=2),
    "depth2": dict(spp=4, max_depth=2, rr_start=3, streams=2),
    "depth255": dict(spp=4, max_depth=255, rr_start=3, streams=2),
    "rr1": dict(spp=4, max_depth=12, rr_start=1, streams=2),
    "rr_never": dict(spp=4, max_depth=24, rr_start=255, streams=2),
    "spp_below_streams": dict(spp=4, max_depth=12, rr_start=3, streams=7),
}


def edge_params(P, key, flags=0):
    return P.make_params(W, H, flags=flags, **EDGE_PARAMS[key])


# the configurations whose next-event frames are compared (tests/test_materials.py, tests/test_gpu_materials.py)
NEE_CONFIGS = [("palette", "front"), ("glass_box", "outside"), ("glass_box", "inside")]


def emissive_triangles(sd):
    """Mask of the triangles SPEC §7 takes as lights: some emission and a positive area, whatever the material's kind."""
    e1, e2 = sd.verts[:, 3:6] - sd.verts[:, 0:3], sd.verts[:, 6:9] - sd.verts[:, 0:3]
    area = 0.5 * np.linalg.norm(np.cross(e1.astype(np.float64), e2.astype(np.float64)), axis=1)
    return sd.mats["emission"][sd.tri_mat].any(axis=1) & (area > 0)
