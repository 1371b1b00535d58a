"""Valid scenes built to reach the corners of the closest-hit code that the generator scenes (scenegen.cpp) leave alone:
traversal stacks deeper than the LDS part, exact ties on t across leaves, zero direction components, rays in the plane of a
wall, long sphere lists, extreme coordinate ranges and rays aimed at the shared edges of a closed mesh. Test helpers only."""
import copy

import numpy as np

LAMBERT, METAL, DIELECTRIC = 0, 1, 2


def _pkg():
    """pathtracing_amd, imported on first use: importing it loads libptrt.so, which a clean checkout only has once the
    session's build fixture has run, and that is after the test modules are collected."""
    import pathtracing_amd
    return pathtracing_amd


def _clone(sd):
    N = _pkg().native
    out = copy.copy(sd)
    for k in ("verts", "tri_mat", "spheres", "sph_mat", "mats", "sky"):
        setattr(out, k, np.array(getattr(sd, k), copy=True))
    out.cam = N.pt_camera.from_buffer_copy(sd.cam)
    return out


def id_scene(sd):
    """The scene with one material per primitive, emission (id + 1, 0, 0), albedo 0 and sky 0, and no pixel jitter: a frame
    of max_depth 1 and spp 1 then holds id + 1 of the closest hit of each camera ray in red (0 for a miss), exactly."""
    P = _pkg()
    out = _clone(sd)
    n = len(sd.tri_mat) + len(sd.sph_mat)
    m = np.zeros(n, P.MATERIAL_DTYPE)
    m["emission"][:, 0] = np.arange(1, n + 1, dtype=np.float32)
    out.mats = m
    out.tri_mat = np.arange(len(sd.tri_mat), dtype=np.uint32)
    out.sph_mat = np.arange(len(sd.tri_mat), n, dtype=np.uint32)
    out.sky = np.zeros(3, np.float32)
    out.cam.jitter = 0
    return out


def ids_of(img):
    """Primitive ids (MISS = 0xFFFFFFFF) from the red channel of an id_scene frame."""
    red = img[..., 0].reshape(-1).astype(np.float64)
    assert (red == np.round(red)).all() and (red >= 0).all()
    return np.where(red == 0, 0xFFFFFFFF, red - 1).astype(np.uint64)


def params_id(w, h, ray_eps=1e-4):
    P = _pkg()
    return P.make_params(w, h, spp=1, max_depth=1, ray_eps=ray_eps)


def stacked_layers(w, h, n=60, ratio=2.0):
    """`n` parallel triangles facing the camera, each covering the whole frame, at distances ratio**i. The binned SAH peels the
    farthest layers off one by one, so every ray's first descent pushes a sibling at every level: deeper than the 12 LDS
    entries for every layout. The layers are glass, so the path tracer's refracted rays take the deep paths again."""
    P = _pkg()
    N = P.native
    sd = P.make_scene(N.PT_SCENE_CORNELL, 0, 1, w, h)
    z0 = float(sd.cam.origin[2])
    verts = []
    for i in range(n):
        dist = ratio ** i
        s = dist * 1.6  # tan(fov/2) = 0.4 and aspect <= 2: the frustum at this distance is inside [-s, s]^2 (wider layers
        #                 change the SAH's splits and give shallower stacks)
        verts.append([-s, -s, z0 - dist, 3 * s, -s, z0 - dist, -s, 3 * s, z0 - dist])
    sd.verts = np.array(verts, np.float32)
    m = np.zeros(n, P.MATERIAL_DTYPE)
    m["kind"] = DIELECTRIC
    m["ior"] = np.linspace(1.2, 1.8, n, dtype=np.float32)
    m["albedo"] = 0.97
    m["emission"][::7, 1] = 0.25
    sd.mats, sd.tri_mat = m, np.arange(n, dtype=np.uint32)
    sd.spheres, sd.sph_mat = sd.spheres[:0], sd.sph_mat[:0]
    sd.sky = np.float32([0.6, 0.7, 1.0])
    return sd


def duplicates(w, h, seed=7):
    """The Cornell box with every triangle repeated 9 to 12 times, the copies scattered over the id range (so a tie on t
    crosses leaves and Morton order) and each copy with its own material."""
    P = _pkg()
    N = P.native
    base = P.make_scene(N.PT_SCENE_CORNELL, 0, 1, w, h)
    rng = np.random.default_rng(seed)
    src = np.concatenate([np.full(9 + i % 4, i) for i in range(len(base.tri_mat))])
    src = src[rng.permutation(len(src))]
    sd = _clone(base)
    sd.verts = base.verts[src].copy()
    n_tri = len(src)
    m = np.concatenate([base.mats[base.tri_mat[src]], base.mats[base.sph_mat]])
    m["albedo"] *= rng.uniform(0.5, 1.0, (len(m), 1)).astype(np.float32)  # every copy looks different
    sd.mats = m
    sd.tri_mat = np.arange(n_tri, dtype=np.uint32)
    sd.sph_mat = np.arange(n_tri, n_tri + len(base.sph_mat), dtype=np.uint32)
    return sd, src


def axis_camera(sd, w, h):
    """An odd frame looking down -z whose centre column and row have direction components of exactly zero: the camera scale
    is a power of two and (cx, cy) is exactly the centre."""
    assert w % 2 == 1 and h % 2 == 1
    out = _clone(sd)
    c = out.cam
    c.forward[:] = (0.0, 0.0, -1.0)
    c.right[:] = (0.4, 0.0, 0.0)
    c.up[:] = (0.0, -0.4, 0.0)
    c.scale = 2.0 ** -5
    c.cx, c.cy = (w / 2) * c.scale, (h / 2) * c.scale
    c.jitter = 0
    return out


def floor_camera(sd, w, h):
    """A camera standing exactly in the plane of the Cornell floor (y = -1), looking along it: the centre row's rays lie in that
    plane (det == 0 for the floor triangles) and the rays below it start on the floor."""
    out = axis_camera(sd, w, h)
    out.cam.origin[:] = (0.0, -1.0, 0.95)
    return out


def sphere_list(n, w, h, seed=3, camera_inside=False):
    """Cornell box with `n` spheres of every material kind (ids after the triangles). camera_inside: sphere 0 is a glass ball
    around the camera, so every camera ray leaves it through the far root (t1)."""
    P = _pkg()
    N = P.native
    sd = P.make_scene(N.PT_SCENE_CORNELL_GLASS, 0, 3, w, h)
    rng = np.random.default_rng(seed + n)
    sph = np.zeros((n, 4), np.float32)
    sph[:, :3] = rng.uniform(-0.8, 0.8, (n, 3))
    sph[:, 3] = rng.uniform(0.04, 0.18, n)
    if camera_inside and n:
        sph[0] = (sd.cam.origin[0], sd.cam.origin[1], sd.cam.origin[2], 0.5)
    base = len(sd.mats)
    m = np.zeros(n, P.MATERIAL_DTYPE)
    m["kind"] = np.arange(n) % 3
    m["albedo"] = rng.uniform(0.3, 0.95, (n, 3)).astype(np.float32)
    m["roughness"] = np.where(np.arange(n) % 2 == 0, 0.0, 0.3)
    m["ior"] = 1.5
    if camera_inside and n:
        m[0]["kind"], m[0]["albedo"] = DIELECTRIC, (0.95, 0.95, 0.95)
    sd.mats = np.concatenate([sd.mats, m])
    sd.spheres, sd.sph_mat = sph, np.arange(base, base + n, dtype=np.uint32)
    return sd


def scaled(sd, k):
    """Every length of the scene times 2**k: vertices, sphere centres and radii, the camera origin (directions keep)."""
    out = _clone(sd)
    s = np.float32(2.0 ** k)
    out.verts = sd.verts * s
    out.spheres = sd.spheres * s
    for i in range(3):
        out.cam.origin[i] = sd.cam.origin[i] * float(s)
    return out


def ray_camera(sd, origin, direction):
    """A 1 x 1 frame whose only camera ray is (origin, normalize(direction)): scale 0 and (cx, cy) = 0 make v = forward."""
    N = _pkg().native
    out = copy.copy(sd)
    c = N.pt_camera()
    c.origin[:] = [float(x) for x in origin]
    c.forward[:] = [float(x) for x in direction]
    c.scale, c.cx, c.cy, c.jitter = 0.0, 0.0, 0.0, 0
    out.cam = c
    return out


def shared_edge_targets(sd, count, seed=2024):
    """`count` points (float32) strictly inside edges that two triangles of the mesh share, from a fixed seed."""
    v = np.asarray(sd.verts, np.float32).reshape(-1, 3, 3)
    keys = {}
    for t in range(len(v)):
        for a, b in ((0, 1), (1, 2), (2, 0)):
            e = tuple(sorted((tuple(v[t, a]), tuple(v[t, b]))))
            keys[e] = keys.get(e, 0) + 1
    shared = sorted(e for e, c in keys.items() if c == 2)
    rng = np.random.default_rng(seed)
    pick = rng.choice(len(shared), count, replace=False)
    f = rng.uniform(0.2, 0.8, count)
    pa = np.array([shared[i][0] for i in pick], np.float64)
    pb = np.array([shared[i][1] for i in pick], np.float64)
    return (pa + f[:, None] * (pb - pa)).astype(np.float32)
