"""What the GPU tests of pt_gather and pt_gather_paths share: the call through the C ABI behind a guard band, comparison bit for bit, the
record of an invalid point and the "other state is untouched" sequence."""
import ctypes as C

import numpy as np

import gather_ref as G

K = G.K
LBVH = 0x100
SKY = np.array([1.0, 2.0, 3.0], np.float32)
SENTINEL = np.array([0, 0, 0, -1, 0, 0, 0, 0], np.float32)


def call(P, r, rec, samples=K, host=True, paths=True, max_depth=8, rr_start=3, n=None, **kw):
    """pt_gather_paths (paths=False: pt_gather) through the C ABI on the first n (default: all) of the (n, 8) records: (out (n, 8) float32,
    pt_stats). host=False: through device tensors. Four rows behind `out` must keep their bytes."""
    N = P.native
    n = len(rec) if n is None else n
    gp = N.pt_gather_params(samples=samples, seed=kw.get("seed", 0), sample_offset=kw.get("sample_offset", 0),
                            point_offset=kw.get("point_offset", 0), max_distance=kw.get("max_distance", 0.0),
                            ray_eps=kw.get("ray_eps", G.EPS), flags=N.PT_GATHER_HOST_MEMORY if host else 0)
    pp = N.pt_gather_path_params(max_depth=max_depth, rr_start=rr_start)
    st = N.pt_stats()
    rec = np.ascontiguousarray(rec, np.float32)
    if host:
        out = np.full((n + 4, 8), 7.0, np.float32)
        a, b = rec.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    else:
        import torch
        d_rec = torch.as_tensor(rec, device="cuda")
        d_out = torch.full((n + 4, 8), 7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        a, b = C.c_void_p(d_rec.data_ptr()), C.c_void_p(d_out.data_ptr())
    if paths:
        rc = N.lib.pt_gather_paths(r._ctx, r._scene, a, b, n, C.byref(gp), C.byref(pp), C.byref(st))
    else:
        rc = N.lib.pt_gather(r._ctx, r._scene, a, b, n, C.byref(gp), C.byref(st))
    assert rc == N.PT_OK, (rc, N.lib.pt_last_error(r._ctx))
    if not host:
        out = d_out.cpu().numpy()
    assert (out[n:] == 7.0).all(), ("guard band", n, samples, out[n:])
    return out[:n], st


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def other_state_is_untouched(P, sd, rec, paths):
    """A PT_FLAG_ACCUMULATE sequence with the call in the middle is the sequence without it, and the framebuffer, the denoised and
    displayed images, the guides and the temporal history of the frame survive the call."""
    N = P.native

    def sequence(with_gather):
        r = P.Renderer(P.Window(G.W, G.H))
        r.Init()
        try:
            r.SetScene(sd, 0)
            r.Params = P.make_params(G.W, G.H, spp=2, max_depth=4, streams=2)
            r.Render(0.0)
            r.Denoise()
            r.DenoiseTemporal()
            r.Display()
            kept = lambda: (r.ReadFramebuffer(), r.ReadDenoised(), r.ReadDisplay().astype(np.float32), r.ReadTemporal(), r.ReadGuides(),
                            r.ReadHistoryLength())
            before = kept()
            if with_gather:
                out, _ = call(P, r, rec, paths=paths)
                assert out[:, 3].min() >= 0, ("an invalid point among the first hits", float(out[:, 3].min()))
                changed = [j for j, (a, b) in enumerate(zip(kept(), before)) if not same(np.asarray(a, np.float32), np.asarray(b, np.float32))]
                assert not changed, ("the call changed (0 framebuffer, 1 denoised, 2 display, 3 temporal, 4 guides, 5 history length)", changed)
            r.Params = P.make_params(G.W, G.H, spp=2, max_depth=4, streams=2, sample_offset=2, flags=N.PT_FLAG_ACCUMULATE)
            st = r.Render(0.0)
            return r.ReadFramebuffer(), int(st.rays)
        finally:
            r.Dispose()

    a, b = sequence(True), sequence(False)
    assert same(a[0], b[0]) and a[1] == b[1], ("the accumulated frame differs", int((bits(a[0]) != bits(b[0])).sum()), a[1], b[1])
