"""CPU-side checks: the C-ABI library loads and exports every symbol include/ptrt.h declares, the host logic
(tile layout, scene generators, argument validation) behaves, and the product refuses to run without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gpu():
    import torch
    return torch.cuda.is_available()


def test_header_symbols_are_exported(P):
    hdr = open(os.path.join(ROOT, "include", "ptrt.h")).read()
    declared = set(re.findall(r"^(?:pt_status|void|uint32_t|const char \*)\s*(pt_[a-z0-9_]+)\(", hdr, re.M))
    assert len(declared) >= 20
    assert declared == set(P.native.SYMBOLS), declared ^ set(P.native.SYMBOLS)
    for name in declared:
        assert hasattr(P.native.lib, name), name
    assert P.native.lib.pt_abi_version() == P.native.PTRT_ABI_VERSION == 2


def test_struct_layouts(P):
    N = P.native
    assert C.sizeof(N.pt_material) == 48 and C.sizeof(N.pt_camera) == 64 and C.sizeof(N.pt_render_params) == 64
    assert P.MATERIAL_DTYPE.itemsize == 48


def test_no_cpu_fallback(P):
    if _gpu():
        pytest.skip("GPU present")
    r = P.Renderer(P.Window(64, 64))
    with pytest.raises(P.PtException) as e:
        r.Init()
    assert e.value.status == P.native.PT_ERR_NO_DEVICE
    assert "no CPU backend" in str(e.value)


def test_product_does_not_reference_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "pathtracing_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".h", ".hip", "Makefile")):
                txt = open(os.path.join(dirpath, f), errors="replace").read()
                assert "pt_oracle" not in txt and "import pto" not in txt and "libpt_oracle" not in txt, f
    for f in ("include/ptrt.h",):
        assert "pt_oracle" not in open(os.path.join(ROOT, f)).read()


def test_device_resources_have_one_owner():
    """Device buffers, events, streams and pinned blocks are held by the owner types of csrc/device_owner.h and by nothing else: no other
    source file of the library releases one, none creates one except on a line whose comment says why, and the two destroy functions
    release nothing by hand (their members do). A resource added to pt_context or pt_scene then cannot be forgotten."""
    csrc = os.path.join(ROOT, "pathtracing_amd", "csrc")
    owner, src = "device_owner.h", {}
    for dirpath, _, files in os.walk(csrc):
        for f in files:
            if f.endswith((".cpp", ".hip", ".h")):
                src[os.path.relpath(os.path.join(dirpath, f), csrc)] = open(os.path.join(dirpath, f), errors="replace").read()
    assert owner in src and len(src) > 10
    for f, txt in src.items():
        if f == owner:
            continue
        for call in ("hipFree(", "hipHostFree(", "hipEventDestroy(", "hipStreamDestroy("):
            assert call not in txt, (f, call)
        for no, line in enumerate(txt.splitlines(), 1):
            for call in ("hipMalloc(", "hipHostMalloc(", "hipEventCreate", "hipStreamCreate"):
                if call in line:
                    assert "//" in line.split(call, 1)[1], (f, no, call, "outside the owners' header and no comment on the line says why")
    for name in ("pt_context_destroy", "pt_scene_destroy"):  # each defined once, in whichever source file
        bodies = [m.group(0) for txt in src.values() for m in re.finditer(r"^void " + name + r"\(.*?^}", txt, re.M | re.S)]
        assert len(bodies) == 1, (name, len(bodies))
        assert ".release(" not in bodies[0] and "delete " in bodies[0], name


def test_environment_changes_no_tree():
    """The library's sources and its header name two environment variables, PTRT_TRACE and PTRT_TIMING (stderr diagnostics), and every
    getenv reads one of them: an exported variable cannot change a tree, a picture or a benchmarked number."""
    allowed = {"PTRT_TRACE", "PTRT_TIMING"}
    csrc = os.path.join(ROOT, "pathtracing_amd", "csrc")
    paths = [os.path.join(d, f) for d, _, files in os.walk(csrc) for f in files if f.endswith((".cpp", ".hip", ".h", "Makefile"))]
    assert len(paths) > 10
    reads = []
    for path in paths + [os.path.join(ROOT, "include", "ptrt.h")]:
        txt = open(path, errors="replace").read()
        named = set(re.findall(r"\bPTRT_[A-Z0-9_]+", txt)) - {"PTRT_H", "PTRT_ABI_VERSION"}
        assert named <= allowed, (path, named - allowed)
        if path.startswith(csrc):
            reads += [(path, m) for m in re.findall(r"getenv\s*\(\s*([^)]*)\)", txt)]
    assert reads and all(arg.strip('"') in allowed for _, arg in reads), reads


@pytest.mark.parametrize("w,h,nr", [(1920, 1080, 1), (1920, 1080, 8), (3840, 2160, 8), (100, 37, 3), (64, 64, 2), (65, 1, 4)])
def test_tile_layout_partitions_the_frame(P, w, h, nr):
    seen = np.zeros(((h + 63) // 64) * ((w + 63) // 64), int)
    for rank in range(nr):
        lay = P.tile_layout(P.make_params(w, h, rank=rank, nranks=nr))
        assert lay.tile_size == 64 and lay.tiles_x == (w + 63) // 64 and lay.tiles_y == (h + 63) // 64
        mine = list(range(rank, lay.n_tiles, nr))
        assert lay.tiles_mine == len(mine) <= lay.tiles_per_rank == -(-lay.n_tiles // nr)
        seen[mine] += 1
    assert (seen == 1).all()


def test_tile_layout_rejects_bad_params(P):
    for kw in (dict(width=0, height=4), dict(width=4, height=4, rank=2, nranks=2), dict(width=40000, height=4)):
        p = P.make_params(kw.pop("width"), kw.pop("height"), **kw)
        with pytest.raises(P.PtException):
            P.tile_layout(p)


def test_scenegen_is_deterministic_and_sized(P):
    N = P.native
    a, b = P.make_scene(N.PT_SCENE_TRIANGLE_SOUP, 1000, 5, 64, 64), P.make_scene(N.PT_SCENE_TRIANGLE_SOUP, 1000, 5, 64, 64)
    c = P.make_scene(N.PT_SCENE_TRIANGLE_SOUP, 1000, 6, 64, 64)
    assert np.array_equal(a.verts, b.verts) and not np.array_equal(a.verts, c.verts)
    assert a.verts.shape == (1000, 9) and np.abs(a.verts).max() <= 1.01 and (a.sky == 1).all()
    ext = a.verts.reshape(-1, 3, 3)
    assert (ext.max(1) - ext.min(1)).max() <= 0.02 + 1e-6
    co = P.make_scene(N.PT_SCENE_CORNELL, 0, 0, 64, 64)
    assert co.verts.shape == (12, 9) and co.spheres.shape == (4, 4) and (co.mats["kind"] == N.PT_LAMBERT).all()
    assert (co.mats["emission"].sum(1) > 0).sum() == 1
    gl = P.make_scene(N.PT_SCENE_CORNELL_GLASS, 0, 0, 64, 64)
    assert set(gl.mats["kind"][gl.sph_mat]) == {N.PT_LAMBERT, N.PT_METAL, N.PT_DIELECTRIC}
    te = P.make_scene(N.PT_SCENE_CORNELL_TESS, 1 << 20, 0, 64, 64)
    k = int(np.floor(np.sqrt((1 << 20) / 10)))
    assert len(te.tri_mat) == 10 * k * k + 2 and abs(len(te.tri_mat) - (1 << 20)) < 8000
    # tessellation covers the same walls: same bounding box and total area as the coarse box
    def area(v):
        t = v.reshape(-1, 3, 3).astype(np.float64)
        return 0.5 * np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1).sum()
    assert abs(area(te.verts) - area(co.verts)) < 1e-3


def test_detached_scene_argument_validation(P):
    from pathtracing_amd.host import build_bvh_detached
    sd = P.make_scene(0, 0, 0, 64, 64)
    bad = P.SceneData(**{**sd.__dict__}); bad.tri_mat = sd.tri_mat.copy(); bad.tri_mat[3] = 99
    with pytest.raises(P.PtException, match="material id"):
        build_bvh_detached(bad)
    bad = P.SceneData(**{**sd.__dict__}); bad.verts = sd.verts.copy(); bad.verts[0, 0] = np.nan
    with pytest.raises(P.PtException, match="non-finite"):
        build_bvh_detached(bad)
    bad = P.SceneData(**{**sd.__dict__}); bad.spheres = sd.spheres.copy(); bad.spheres[0, 3] = 0.0
    with pytest.raises(P.PtException, match="radius"):
        build_bvh_detached(bad)
    with pytest.raises(P.PtException, match="bvh_width"):
        build_bvh_detached(sd, 3)
    empty = P.SceneData(cam=sd.cam)
    info, nodes, tris = build_bvh_detached(empty)
    assert info.n_nodes == 0 and info.n_tris == 0 and nodes.size == 0
