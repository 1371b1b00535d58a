"""Scenes and blob access for the tests of the builders and the refit (tests/test_gpu_lbvh.py, tests/test_gpu_update.py,
tests/test_gpu_blob_ref.py and the digest tests): the small named scenes of the GPU builder's tests with their reference trees, the
read-out of the device's binary tree, a copy of the committed blob, and moved and deformed geometry for a refit. Test helpers only."""
import ctypes as C
import dataclasses

import numpy as np

import adversarial_scenes as S
import lbvh_ref as L
from trace_support import H, W

F = np.float32


def _random(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, (n, 1, 3)) + rng.uniform(-0.15, 0.15, (n, 3, 3))).astype(F).reshape(n, 9)


def _centred(centres, sizes):
    """Triangles whose unpadded box is centre -+ size exactly (dyadic numbers), so that 0.5 * (lo + hi) is the centre bit for bit."""
    c, a = np.asarray(centres, F).reshape(-1, 3), np.asarray(sizes, F).reshape(-1, 1)
    sign = F([[-1, -1, -1], [1, -1, 1], [-1, 1, 1]])
    return (c[:, None, :] + a[:, None, :] * sign[None]).astype(F).reshape(-1, 9)


def _same(n):
    return _centred(np.tile(F([0.25, -0.5, 0.125]), (n, 1)), (np.arange(n) % 16 + 1) / 64)


def _planar(k=10):
    """2 k^2 triangles of a k x k grid in the plane z = -0.5: no extent in z."""
    g = np.linspace(-0.75, 0.75, k + 1).astype(F)
    out = []
    for i in range(k):
        for j in range(k):
            a, b, c, d = (g[i], g[j]), (g[i + 1], g[j]), (g[i + 1], g[j + 1]), (g[i], g[j + 1])
            out += [[*a, -0.5, *b, -0.5, *c, -0.5], [*a, -0.5, *c, -0.5, *d, -0.5]]
    return F(out)


RANDOM_N = (2, 3, 4, 5, 31, 32, 33, 64, 255, 256, 257, 1023, 1025)
SAME_N = (2, 3, 7, 256, 300)
GENERATED = {"soup3000": ("PT_SCENE_TRIANGLE_SOUP", 3000), "tess2000": ("PT_SCENE_CORNELL_TESS", 2000), "cornell": ("PT_SCENE_CORNELL", 0)}
NAMES = [f"random{n}" for n in RANDOM_N] + list(GENERATED) + [f"same{n}" for n in SAME_N] + \
    ["two_positions", "planar", "at_minus_1e4", "at_plus_1e4", "duplicates", "layers"]


_cache = {}


def scene(P, name):
    """name -> (SceneData, reference tree, reference leaves), made once."""
    if name in _cache:
        return _cache[name]
    N = P.native
    if name in GENERATED:
        sd = P.make_scene(getattr(N, GENERATED[name][0]), GENERATED[name][1], 3, W, H)
    elif name == "duplicates":
        sd = S.duplicates(W, H)[0]
    elif name == "layers":
        sd = S.stacked_layers(W, H)
    else:
        if name.startswith("random"):
            verts = _random(int(name[6:]), int(name[6:]))
        elif name.startswith("same"):
            verts = _same(int(name[4:]))
        elif name == "two_positions":
            verts = _centred(np.where(np.arange(300)[:, None] % 2 == 0, F([-0.5, 0.25, -0.25]), F([0.5, 0.25, 0.5])), (np.arange(300) % 8 + 1) / 32)
        elif name == "planar":
            verts = _planar()
        else:
            verts = (_random(300, 5).reshape(-1, 3) * F(0.5) + F(-1e4 if "minus" in name else 1e4)).astype(F).reshape(-1, 9)
        sd = S._clone(P.make_scene(N.PT_SCENE_CORNELL, 0, 1, W, H))
        sd.verts = verts
        sd.tri_mat = (np.arange(len(verts)) % len(sd.mats)).astype(np.uint32)
    tree = L.build(sd.verts)
    _cache[name] = (sd, tree, L.leaf_partition(tree)[0])
    return _cache[name]


def readout(P, r, verts):
    """The binary tree of build_lbvh_device through the test-only entry point: dict of order, left, right, first, last, box."""
    v = np.ascontiguousarray(verts, F).reshape(-1, 9)
    n = len(v)
    t = dict(order=np.full(n, 0xFFFFFFFF, np.uint32), left=np.zeros(n - 1, np.int32), right=np.zeros(n - 1, np.int32),
             first=np.zeros(n - 1, np.uint32), last=np.zeros(n - 1, np.uint32), box=np.zeros((n - 1, 6), F))
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    st = P.native.lib.pt_internal_lbvh_binary(r._ctx, p(v), n, p(t["order"]), p(t["left"]), p(t["right"]), p(t["first"]), p(t["last"]), p(t["box"]))
    assert st == P.native.PT_OK, P.native.lib.pt_last_error(r._ctx)
    return t


def blob(r):
    info = r.BvhInfo()
    nodes, tris = r.BvhRead()
    return info, nodes.copy(), tris.copy()


SCENES = ["cornell", "glass", "tess", "soup", "layers", "duplicates", "spheres64"]


def moved(sd, verts=None, spheres=None):
    return dataclasses.replace(sd, verts=sd.verts if verts is None else np.asarray(verts, np.float32).reshape(-1, 9),
                               spheres=sd.spheres if spheres is None else np.asarray(spheres, np.float32).reshape(-1, 4))


def deform(sd, rng, kind):
    """'small': every vertex jittered by 1e-3 of the scene's extent; 'large': every triangle carried up to 40 % of the extent across
    the scene (plus jitter), so that leaves overlap and boxes grow."""
    v = np.asarray(sd.verts, np.float32).reshape(-1, 3, 3)
    if len(v) == 0:
        return np.zeros((0, 9), np.float32)
    ext = float(np.ptp(v.reshape(-1, 3), axis=0).max())
    out = v.astype(np.float64) + rng.normal(scale=1e-3 * ext, size=v.shape)
    if kind == "large":
        out += rng.uniform(-0.4 * ext, 0.4 * ext, size=(len(v), 1, 3))
    return out.astype(np.float32).reshape(-1, 9)
