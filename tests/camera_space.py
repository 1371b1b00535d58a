"""The cases of the camera space, stated once for tests/test_camera_space.py (no device) and tests/test_gpu_camera_space.py:
named cameras that leave the family every other test stays in (right, up and forward orthogonal, |right| = |up|, |forward| = 1, the
principal point in the image centre), the scenes they look at, a float64 restatement of §3's camera ray and of DESIGN.md's
"Sky pixels: The bound", and the decoder of the rectangle a frame reports in pt_stats.reserved[3]. Test helpers only.

Pytest rewrites `assert` only in test modules, so every assert here carries its own message."""
import copy
import dataclasses

import numpy as np

import ray_caster64 as rc
import temporal_cases as tc

SKY = np.float32([0.3, 0.5, 0.9])  # (the generator scenes' own sky is black: a sky pixel would look like an unlit one)
W, H = 64, 48
ALL_SKY = "all sky"

RESOLVING = ("default", "rolled", "off_centre", "anisotropic", "skewed", "long_forward", "narrow", "left_handed", "mirrored", "zoom_edge",
             "wide", "far", "shifted_world", "no_jitter", "corner_on_threshold_in")
GIVE_UP = ("inside", "behind", "beside_plane", "beside_wide", "corner_on_threshold_out", "scale_zero", "scale_negative", "flat_basis")
CASE_NAMES = RESOLVING + GIVE_UP
TEMPORAL_CASES = ("rolled", "skewed", "anisotropic", "off_centre", "left_handed", "mirrored")

# name -> (what make_scene or this module builds, the layout it is committed in); Cornell's default layout is BVH2
SCENES = {"cornell": ("PT_SCENE_CORNELL", 0), "tess68": ("PT_SCENE_CORNELL_TESS", 68), "tess72": ("PT_SCENE_CORNELL_TESS", 72),
          "tess73": ("PT_SCENE_CORNELL_TESS", 73), "spheres": ("spheres_only", 0), "triangle": ("one_triangle", 0)}


# ------------------------------------------------------------------------------------------------ scenes

def scene_of(P, kind, w, h, seed=5):
    return dataclasses.replace(P.make_scene(getattr(P.native, kind), 3000 if kind == "PT_SCENE_CORNELL_TESS" else 0, seed, w, h), sky=SKY)


def spheres_only(P, w, h):
    """Spheres and no triangle: one in the middle, one across the left border of the image, one across its top, and a small one far
    away whose test is the least exact."""
    sd = scene_of(P, "PT_SCENE_CORNELL", w, h)
    sph = np.array([[0.0, 0.0, 0.0, 0.45], [-1.9, 0.1, -0.5, 0.5], [0.4, 1.35, -0.3, 0.3], [0.9, -0.6, -30.0, 0.12]], np.float32)
    return P.SceneData(spheres=sph, sph_mat=np.zeros(len(sph), np.uint32), mats=sd.mats, cam=sd.cam, sky=sd.sky)


def one_triangle(P, w, h):
    """One small triangle, tilted against every axis, around the point the generator camera looks at."""
    sd = scene_of(P, "PT_SCENE_CORNELL", w, h)
    verts = np.array([[-1.2, -0.8, 0.5, 0.9, -0.5, -0.6, 0.1, 1.0, 0.2]], np.float32)
    return P.SceneData(verts=verts, tri_mat=np.zeros(1, np.uint32), mats=sd.mats, cam=sd.cam, sky=sd.sky)


def scene(P, name, w=W, h=H):
    """(scene data under the generator camera, layout) of SCENES[name]."""
    kind, layout = SCENES[name]
    sd = spheres_only(P, w, h) if kind == "spheres_only" else one_triangle(P, w, h) if kind == "one_triangle" else scene_of(P, kind, w, h)
    return sd, layout


def empty_like(P, sd):
    return P.SceneData(mats=sd.mats, cam=sd.cam, sky=sd.sky)


def sky_mask(P, pto, sd, params, bvh=None):
    """Per the oracle alone: the pixels of the frame `params` of `sd` whose every sample missed. They show exactly the value of the
    same frame of the empty scene; with max_depth = 1 no other pixel does (a hit adds its emission, a miss the sky, with weight 1)."""
    ref, _ = pto.render(pto.Scene(sd, bvh), params)
    void, _ = pto.render(pto.Scene(empty_like(P, sd)), params)
    return (ref == void).all(axis=2)


# ------------------------------------------------------------------------------------------------ cameras

def turned(sd, yaw, shift=(0.0, 0.0, 0.0)):
    """sd with its camera turned about the y axis by `yaw` radians and moved by `shift`."""
    sd = copy.copy(sd)
    cam = type(sd.cam)()
    cam.scale, cam.cx, cam.cy, cam.jitter = sd.cam.scale, sd.cam.cx, sd.cam.cy, sd.cam.jitter
    c, s = np.cos(yaw), np.sin(yaw)
    for k in range(3):
        cam.origin[k] = sd.cam.origin[k] + shift[k]
    for name in ("forward", "right", "up"):
        v = getattr(sd.cam, name)
        out = (c * v[0] + s * v[2], v[1], -s * v[0] + c * v[2])
        for k in range(3):
            getattr(cam, name)[k] = out[k]
    sd.cam = cam
    return sd


class Cam64:
    """A camera's sixteen words in float64."""

    def __init__(self, cam):
        self.o, self.f, self.r, self.u = (np.array(v[:], np.float64) for v in (cam.origin, cam.forward, cam.right, cam.up))
        self.scale, self.cx, self.cy, self.jitter = float(cam.scale), float(cam.cx), float(cam.cy), int(cam.jitter)

    def stored(self, like):
        """The pt_camera that holds these words as float32."""
        cam = type(like)()
        cam.origin[:], cam.forward[:], cam.right[:], cam.up[:] = self.o.tolist(), self.f.tolist(), self.r.tolist(), self.u.tolist()
        cam.scale, cam.cx, cam.cy, cam.jitter = self.scale, self.cx, self.cy, self.jitter
        return cam


def _rot(v, axis, angle):
    k = axis / np.linalg.norm(axis)
    return v * np.cos(angle) + np.cross(k, v) * np.sin(angle) + k * np.dot(k, v) * (1.0 - np.cos(angle))


def _turn(c, axis, angle):
    c.f, c.r, c.u = (_rot(v, axis, angle) for v in (c.f, c.r, c.u))


def _bounds64(sd):
    """The float64 bounding box of sd's vertices and spheres."""
    v = np.asarray(sd.verts, np.float64).reshape(-1, 3)
    s = np.asarray(sd.spheres, np.float64).reshape(-1, 4)
    lo = np.concatenate([v, s[:, :3] - s[:, 3:]]).min(axis=0)
    hi = np.concatenate([v, s[:, :3] + s[:, 3:]]).max(axis=0)
    return lo, hi


def _corners(lo, hi):
    return np.array([[(hi if i & 1 else lo)[0], (hi if i & 2 else lo)[1], (hi if i & 4 else lo)[2]] for i in range(8)])


def _silhouette(sd, c, w, h):
    """(sx, sy) of a point on the right-hand silhouette of the scene under camera c: on the image row nearest the middle that shows
    the scene, the boundary between its last hit and the sky to the right of it, bisected with the float64 caster."""

    def hit(px, py):
        sx, sy = px * c.scale - c.cx, py * c.scale - c.cy
        d = c.f + sx * c.r + sy * c.u
        return rc.cast(sd.verts, sd.spheres, c.o[None].astype(np.float32), (d / np.linalg.norm(d))[None].astype(np.float32))[0][0] != rc.MISS

    for y in sorted(range(h), key=lambda y: abs(y + 0.5 - h / 2)):
        xs = [x for x in range(w) if hit(x + 0.5, y + 0.5)]
        if xs:
            break
    assert xs, "camera_space._silhouette: the scene is nowhere in the generator camera's image"
    a, b = xs[-1] + 0.5, xs[-1] + 1.5  # hit at a; a miss at b, or the image ends there
    if hit(b, y + 0.5):
        a = b = float(w)  # the scene runs off the image: aim at the image's border, where the root's boxes end further out
    for _ in range(30):
        m = 0.5 * (a + b)
        a, b = (m, b) if hit(m, y + 0.5) else (a, m)
    return a * c.scale - c.cx, (y + 0.5) * c.scale - c.cy


def cases(P, sd, w=W, h=H):
    """{name: scene data} for every name of CASE_NAMES: sd under a camera derived in float64 from sd's own (the generator's) and stored
    as float32; `shifted_world` moves the scene too. The resolving cases show the scene and the sky; the rule of DESIGN.md
    "Sky pixels" gives up on the others."""
    g = Cam64(sd.cam)
    fh = g.f / np.linalg.norm(g.f)
    lo, hi = _bounds64(sd)
    look_at = np.zeros(3)  # the generator camera looks at the world's origin, where every scene here has its middle
    out = {}

    def put(name, c, scene=sd):
        out[name] = dataclasses.replace(scene, cam=c.stored(sd.cam))

    put("default", g)

    c = copy.deepcopy(g)  # the box's silhouette is not axis-aligned on screen
    _turn(c, c.f, np.radians(37.0))
    _turn(c, np.array([0.0, 1.0, 0.0]), 0.12)
    _turn(c, c.r, -0.08)
    put("rolled", c)

    c = copy.deepcopy(g)  # the principal point at (-0.3 w, 1.4 h); the origin moved so that the scene's middle shows at (0.4 w, 0.5 h)
    c.cx, c.cy = -0.3 * w * c.scale, 1.4 * h * c.scale
    depth = float(np.dot(look_at - c.o, fh)) / np.linalg.norm(c.f)
    c.o = c.o - 0.7 * w * c.scale * depth * c.r + 0.9 * h * c.scale * depth * c.u
    put("off_centre", c)

    c = copy.deepcopy(g)
    c.r, c.u = 2.0 * c.r, 0.5 * c.u
    put("anisotropic", c)

    c = copy.deepcopy(g)  # no pair is orthogonal
    c.r = c.r + 0.3 * c.u
    c.f = c.f + 0.2 * c.r + 0.1 * c.u
    put("skewed", c)

    c = copy.deepcopy(g)  # the same picture
    c.f, c.r, c.u = 8.0 * c.f, 8.0 * c.r, 8.0 * c.u
    put("long_forward", c)

    c = copy.deepcopy(g)  # an eighth of the field of view from eight times as far: about the same size, all but parallel rays
    c.f = 8.0 * c.f
    c.o = c.o - 7.0 * np.linalg.norm(c.o) * fh
    put("narrow", c)

    for name, v in (("left_handed", "u"), ("mirrored", "r")):  # det changes sign; seen from the side, so that the picture is not symmetric
        c = Cam64(turned(sd, 0.15, (0.5, 0.2, 0.0)).cam)
        setattr(c, v, -getattr(c, v))
        put(name, c)

    c = copy.deepcopy(g)  # 64 x: a pixel of the default image fills the frame, the silhouette runs through it off the pixel grid
    sx, sy = _silhouette(sd, g, w, h)
    c.scale = g.scale / 64.0
    c.cx, c.cy = (0.5 * w + 0.37) * c.scale - sx, (0.5 * h + 0.21) * c.scale - sy
    put("zoom_edge", c)

    c = copy.deepcopy(g)  # six times the field of view, from 0.6 in front of the scene's nearest corner
    c.r, c.u = 6.0 * c.r, 6.0 * c.u
    c.o = c.o + (min(float(np.dot(p - c.o, fh)) for p in _corners(lo, hi)) - 0.6) * fh
    put("wide", c)

    c = copy.deepcopy(g)  # 1000 units further back; a pixel is 0.1 units wide at the scene: a box of 2 spans 20 pixels
    c.o = c.o - 1000.0 * fh
    c.scale = 0.1 / (np.linalg.norm(g.r) * float(np.dot(look_at - c.o, fh)))
    c.cx, c.cy = 0.5 * w * c.scale, 0.5 * h * c.scale
    put("far", c)

    c = copy.deepcopy(g)
    shift = np.array([3000.0, -2000.0, 1000.0])
    c.o = c.o + shift
    moved = dataclasses.replace(sd, verts=(np.asarray(sd.verts, np.float64).reshape(-1, 3, 3) + shift).reshape(-1, 9).astype(np.float32),
                                spheres=(np.asarray(sd.spheres, np.float64).reshape(-1, 4) + np.append(shift, 0.0)).astype(np.float32))
    put("shifted_world", c, moved)

    c = copy.deepcopy(g)
    c.jitter = 0
    put("no_jitter", c)

    # the three situations of test_camera_inside_and_scene_behind: inside the scene's box; in front of it, turned aside; behind it
    out["inside"] = turned(sd, 0.0, (0.0, 0.0, -3.2))
    out["beside_plane"] = turned(sd, 1.2, (0.0, 0.0, -2.2))
    out["behind"] = turned(sd, 0.0, (0.0, 0.0, -5.5))

    # beside the scene, looking past it with six times the field of view: the corners nearest the camera plane are behind it, and
    # projected anyway they land on the far side of the image, away from the part of the scene that is in view
    c = copy.deepcopy(g)
    c.r, c.u = 6.0 * c.r, 6.0 * c.u
    c.o = np.array([hi[0] + 2.0, 0.5 * (lo[1] + hi[1]), hi[2] - 0.5])
    put("beside_wide", c)

    # The default picture through a sheared camera: forward' = forward + K right', cx' = cx + K. A point's coefficients become
    # a' = a - K c, b' = b, c' = c, so c / (|a'| + |b'| + |c'|) is about 1 / K at every corner: just above the rule's 1e-4 with
    # K = 9900, just below it with K = 10100 (|a / c| and |b / c| stay below 99 in every scene here). right, up / 8 and scale * 8 keep
    # the rule's margin of 1e-4 |cx / scale| = 1e-4 K / scale at 3 pixels.
    for name, K in (("corner_on_threshold_in", 9900.0), ("corner_on_threshold_out", 10100.0)):
        c = copy.deepcopy(g)
        c.r, c.u, c.scale, c.cx, c.cy = c.r / 8.0, c.u / 8.0, 8.0 * c.scale, 8.0 * c.cx, 8.0 * c.cy
        c.f = c.f + K * c.r
        c.cx = c.cx + K
        put(name, c)

    c = copy.deepcopy(g)
    c.scale = 0.0
    put("scale_zero", c)
    c = copy.deepcopy(g)
    c.scale = -g.scale
    put("scale_negative", c)
    c = copy.deepcopy(g)  # det = 0
    c.u = 0.5 * c.r
    put("flat_basis", c)

    assert tuple(sorted(out)) == tuple(sorted(CASE_NAMES)), ("camera_space.cases", sorted(out), sorted(CASE_NAMES))
    return {name: out[name] for name in CASE_NAMES}


def camera_pair(P, sd, name, w=W, h=H):
    """(old scene data, new scene data) of a temporal camera pair: case `name`'s camera, and that camera moved by move_camera."""
    old = cases(P, sd, w, h)[name]
    return old, tc.with_camera(old, tc.move_camera(old.cam, 0.03, 1.5, offset=(0.0, 0.01, 0.0)))


# ------------------------------------------------------------------------------------------------ §3 in float64

def camera_dir64(cam, x, y, jx=0.5, jy=0.5):
    """docs/SPEC.md §3 evaluated in float64 on the camera's float32 words: the unnormalised vector v of pixel (x, y) at jitter
    (jx, jy), and (sx, sy, tx, ty) with tx = (x + jx) scale, ty = (y + jy) scale."""
    c = Cam64(cam)
    tx, ty = (x + jx) * c.scale, (y + jy) * c.scale
    sx, sy = tx - c.cx, ty - c.cy
    return c.f + sx * c.r + sy * c.u, (sx, sy, tx, ty)


# ------------------------------------------------------------------------------------------------ the rule, restated

VARIANTS = ("no_inverse", "cx_sign", "ab_swapped", "lengths_ignored", "behind_projected", "no_sphere_boxes", "no_margins")


def root_slots(layout, nodes):
    """The root's child boxes as the device holds them: node 0 of the blob, decoded per layout. A scene without triangles has none."""
    nodes = np.asarray(nodes, np.uint8)
    return rc._node_slots(layout, nodes, 0) if nodes.size else []


def scene_rect64(slots, spheres, cam, w, h, variant=None):
    """DESIGN.md "Sky pixels: The bound" in plain float64, written from that text. Returns (result, sides): result is None (nothing
    can be said, or the rectangle holds the whole image: nothing to resolve), ALL_SKY (every pixel can be resolved) or the rectangle
    (x0, x1, y0, y1) of pixels x0 <= x < x1, y0 <= y < y1 outside of which every pixel is sky; sides are the four real-valued sides
    (X0, X1, Y0, Y1) before floor and ceil, None where the rule never got that far.

    `variant`: one of VARIANTS, a deliberately wrong rule for the negative controls."""
    assert variant is None or variant in VARIANTS, ("scene_rect64: unknown variant", variant)
    c = Cam64(cam)
    margins = variant != "no_margins"
    boxes = [(np.asarray(lo, np.float64), np.asarray(hi, np.float64)) for lo, hi, _ in slots]
    if variant != "no_sphere_boxes":
        for s in np.asarray(spheres, np.float32).reshape(-1, 4).astype(np.float64):
            r = np.sqrt(s[3] ** 2 + 2.0 ** -16 * (np.linalg.norm(s[:3] - c.o) + s[3]) ** 2) if margins else s[3]
            boxes.append((s[:3] - r, s[:3] + r))
    if not boxes:
        return ALL_SKY, None
    lo, hi = np.min([b[0] for b in boxes], axis=0), np.max([b[1] for b in boxes], axis=0)
    big = max(np.abs(lo).max(), np.abs(hi).max(), np.abs(c.o).max())
    if not big < 1e15:
        return None, None
    if margins:
        lo, hi = lo - 1e-4 * big, hi + 1e-4 * big
    det = np.linalg.det(np.stack([c.r, c.u, c.f], axis=1))
    if not abs(det) > 1e-6 * np.linalg.norm(c.r) * np.linalg.norm(c.u) * np.linalg.norm(c.f) or not c.scale > 0.0:
        return None, None
    px, py = [], []
    for p in _corners(lo, hi):
        v = p - c.o
        if variant == "no_inverse":  # right for an orthogonal basis only
            a, b, d = np.dot(v, c.r) / np.dot(c.r, c.r), np.dot(v, c.u) / np.dot(c.u, c.u), np.dot(v, c.f) / np.dot(c.f, c.f)
        elif variant == "lengths_ignored":  # right for unit vectors only
            a, b, d = np.linalg.solve(np.stack([c.r / np.linalg.norm(c.r), c.u / np.linalg.norm(c.u), c.f / np.linalg.norm(c.f)], axis=1), v)
        else:
            a, b, d = np.linalg.solve(np.stack([c.r, c.u, c.f], axis=1), v)
        if variant == "ab_swapped":
            a, b = b, a
        if not d > 1e-4 * (abs(a) + abs(b) + abs(d)) and variant != "behind_projected":
            return None, None
        px.append((a / d + (-c.cx if variant == "cx_sign" else c.cx)) / c.scale)
        py.append((b / d + (-c.cy if variant == "cx_sign" else c.cy)) / c.scale)
    mx = 1.0 + 1e-4 * (w + abs(c.cx / c.scale)) if margins else 0.0
    my = 1.0 + 1e-4 * (h + abs(c.cy / c.scale)) if margins else 0.0
    sides = (min(px) - mx, max(px) + mx, min(py) - my, max(py) + my)
    if not np.isfinite(sides).all():
        return None, None
    # a pixel is sky only if its whole footprint [x, x + 1) lies outside: x + 1 <= X0 or x >= X1
    x0, x1 = int(np.clip(np.floor(sides[0]), 0, w)), int(np.clip(np.ceil(sides[1]), 0, w))
    y0, y1 = int(np.clip(np.floor(sides[2]), 0, h)), int(np.clip(np.ceil(sides[3]), 0, h))
    if x0 >= x1 or y0 >= y1:
        return ALL_SKY, sides
    if (x0, x1, y0, y1) == (0, w, 0, h):
        return None, sides
    return (x0, x1, y0, y1), sides


def tied(sides, w, h, eps=1e-6):
    """Whether a real-valued side lies within eps of an integer at which floor or ceil could fall either way: one of 0 .. n."""
    if sides is None:
        return False
    return any(abs(s - round(s)) <= eps and -1 <= round(s) <= n + 1 for s, n in zip(sides, (w, w, h, h)))


def unsound(result, sky):
    """The pixels that `result` (of scene_rect64) would resolve although, per the oracle's mask `sky`, a sample of theirs hit."""
    if result is None:
        return np.zeros((0, 2), int)
    outside = np.ones(sky.shape, bool)
    if result != ALL_SKY:
        x0, x1, y0, y1 = result
        outside[y0:y1, x0:x1] = False
    return np.argwhere(outside & ~sky)


def reported_rect(stats):
    """pt_stats.reserved[3] of a non-counting frame (include/ptrt.h), decoded as scene_rect64 states its result."""
    code = int(stats.reserved[3])
    if code == 0:
        return None
    if code == (1 << 64) - 1:
        return ALL_SKY
    return code & 0xFFFF, code >> 16 & 0xFFFF, code >> 32 & 0xFFFF, code >> 48 & 0xFFFF
