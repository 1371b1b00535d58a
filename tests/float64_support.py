"""What the float64 tests of the closest hit share (tests/test_geometry_float64.py, tests/test_gpu_geometry.py and others): the
adversarial scene dictionary at its frame sizes, the host builder on a detached scene, the classification check against the caster
(tests/ray_caster64.py) and the shared-edge rays. Test helpers only."""
import numpy as np

import adversarial_scenes as S
import ray_caster64 as rc

W, H = 65, 49           # odd: the axis camera's centre row and column
CRACK_RAYS = 300        # rays aimed at interior points of shared edges of the tessellated Cornell box
PINNED_CRACKS = 44      # of them, the rays SPEC §4's Möller–Trumbore lets through (brute force and BVH alike)
ALLOWED = 0.01          # the edge and coincident classes together stay below this fraction of a frame's pixels


def build_bvh_detached(scene, layout=0):
    """The product's host builder on a detached scene. Imported late: libptrt.so exists only once the build fixture has run,
    after collection."""
    from pathtracing_amd.host import build_bvh_detached as build
    return build(scene, layout)


def oracle_ids(pto, sd, layout, w, h):
    sd = S.id_scene(sd)
    info, nodes, tris = build_bvh_detached(sd, layout)
    img, _ = pto.render(pto.Scene(sd, (info.width, nodes, tris)), S.params_id(w, h))
    return S.ids_of(img)


def scenes(P, w=W, h=H):
    N = P.native
    c1 = P.make_scene(N.PT_SCENE_CORNELL, 0, 1, w, h)
    return {
        "tess": P.make_scene(N.PT_SCENE_CORNELL_TESS, 2000, 5, w + 1, h + 1),
        "c4": P.make_scene(N.PT_SCENE_CORNELL_GLASS, 0, 5, w, h),
        "layers": S.stacked_layers(w, h),
        "duplicates": S.duplicates(w, h)[0],
        "axis": S.axis_camera(c1, w, h),
        "floor": S.floor_camera(c1, w, h),
        "spheres64": S.sphere_list(64, w, h),
        "inside_sphere": S.sphere_list(31, w, h, camera_inside=True),
    }


def check_classes(sd, o, d, ids, name, cast_result=None):
    """Assert the classification of `ids` against the caster; returns the classes."""
    c = rc.classify(sd.verts, sd.spheres, o, d, ids, cast_result)
    n = {k: len(v) for k, v in c.items() if k != "want"}
    assert n["wrong"] == 0, (name, n, c["wrong"][:10], ids[c["wrong"][:10]], c["want"][c["wrong"][:10]])
    assert n["edge"] + n["coincident"] <= ALLOWED * len(o), (name, n)
    return c


# the frame size the tessellated scene is checked at: its regular grid lines up with every 4th pixel column of a 65-wide frame
def _size(name):
    return (W + 1, H + 1) if name == "tess" else (W, H)


def crack_rays(P, pto):
    """The tessellated Cornell box (30,000 triangles, 160x120 camera) and CRACK_RAYS rays from its camera to shared-edge points,
    each as the only pixel of a 1x1 camera (so the device can trace exactly these rays)."""
    sd = P.make_scene(P.native.PT_SCENE_CORNELL_TESS, 30000, 0x5EED0001, 160, 120)
    org = np.array(sd.cam.origin[:], np.float32)
    cams = [S.ray_camera(sd, org, p - org) for p in S.shared_edge_targets(sd, CRACK_RAYS)]
    rays = [pto.camera_ray(c.cam, 0, 0) for c in cams]
    return sd, cams, np.array([r[0] for r in rays]), np.array([r[1] for r in rays])
