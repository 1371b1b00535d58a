"""Developer aid: what a textured frame costs. 1080p / 64 spp, 8 streams, depth 8, a 1024 x 1024 texture on every wall of
the Cornell box (12 triangles, and tessellated to 1M), plain and with PT_FLAG_NEXT_EVENT, against the same scene untextured on its default
pipeline and forced onto the kernel textured frames run on (pt_tuning.extend_kernel = 1). Median, min and max of 9 warm frames each.
usage: python tools/exp_textures.py [out.json]   (default: tex_cost.json in the working directory)"""
import dataclasses, json, os, sys, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pathtracing_amd as P


def planar_uvs(verts, scale, offset):
    """(triangles, 6): every vertex projected along its triangle's dominant normal axis."""
    v = np.asarray(verts, np.float32).reshape(-1, 3, 3)
    axis = np.abs(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])).argmax(1)
    uv = np.zeros((len(v), 3, 2), np.float32)
    for a in range(3):
        keep = [k for k in range(3) if k != a]
        uv[axis == a] = v[axis == a][:, :, keep] * np.float32(scale) + np.asarray(offset, np.float32)
    return uv.reshape(-1, 6)


def textured(sd, tex, bound):
    mt = np.full(len(sd.mats), P.native.PT_NO_TEXTURE, np.uint32)
    mt[list(bound)] = 0
    return dataclasses.replace(sd, uvs=planar_uvs(sd.verts, 0.5, (0.5, 0.5)), textures={0: tex}, material_textures=mt)


N = P.native
W, H, SPP, REPS = 1920, 1080, 64, 9
r = P.Renderer(P.Window(W, H)); r.Init()
rng = np.random.default_rng(1)
tex = (0.2 + 0.8 * rng.random((1024, 1024, 3))).astype(np.float32)
out = {}
for name, kind, detail in (("cornell", N.PT_SCENE_CORNELL, 0), ("cornell_tess_1M", N.PT_SCENE_CORNELL_TESS, 1 << 20)):
    plain = P.make_scene(kind, detail, 0x5EED0001, W, H)
    # one repeat per wall: s, t in [0, 1] over the [-1, 1] box
    tsd = textured(plain, tex, (0, 1, 2))
    for nee in (False, True):
        ms = {"plain_default": [], "plain_simple": [], "textured": []}
        rays = {}
        params = P.make_params(W, H, spp=SPP, max_depth=8, streams=8, next_event=nee)
        for variant, sd, k in (("plain_default", plain, 0), ("plain_simple", plain, 1), ("textured", tsd, 0)):
            r.SetTuning(extend_kernel=k)
            r.SetScene(sd, 0)
            r.Params = params
            for i in range(REPS + 3):
                st = r.Render(0.0)
                if i >= 3:
                    ms[variant].append(st.gpu_ms)
            rays[variant] = int(st.rays)
            assert variant != "textured" or st.reserved[0] == 1
        r.SetTuning(extend_kernel=0)
        row = {v: {"median_ms": statistics.median(x), "min_ms": min(x), "max_ms": max(x), "rays": rays[v]} for v, x in ms.items()}
        out[f"{name}{'+nee' if nee else ''}"] = row
        print(name, "nee" if nee else "plain", json.dumps(row), flush=True)
info = r.TextureInfo(0)
out["texture_device_bytes"] = int(info.device_bytes)
json.dump(out, open(sys.argv[1] if len(sys.argv) > 1 else "tex_cost.json", "w"), indent=1)
r.Dispose()
