"""The brute-force float64 path tracer of the physics pin (tests/test_physics_pin.py holds the oracle to it, tests/test_gpu_parity.py
the device): numpy's RNG, its own hemisphere parametrisation and intersection code, no routine shared with either implementation.
Test helpers only."""
import numpy as np


def numpy_radiance(sd, width, height, n_paths, max_depth, rr_start, rng, drop_cosine=False, own_roulette=False, wrong=None):
    """Mean radiance and standard error per pixel of a width x height frame: float64, numpy RNG, brute-force intersection of every
    triangle and sphere, implicit light hits only, the depth cut of docs/SPEC.md §5 (it is part of the expectation).
    Surfaces are evaluated from the physics, not with the spec's sampling routines: Lambert by cosine sampling in an own
    parametrisation; rough metal by sampling the GGX normal distribution D(h) cos(theta_h) (Walter et al. 2007 — the spec and both
    implementations use Heitz's visible-normal sampling) and weighting with BRDF * cos / pdf; mirror and glass by Snell / exact
    unpolarised Fresnel. `own_roulette`: Russian roulette with a constant survival probability of 0.85 instead of the spec's
    throughput-dependent one (any roulette leaves the expectation alone, so this checks the spec's for bias).
    `drop_cosine`: sample the hemisphere uniformly WITHOUT the 2 cos weight; `wrong="no_masking"`: leave the Smith terms out of the
    metal weight; `wrong="no_reflection"`: glass always refracts (deliberately wrong estimators, to show the comparisons have teeth)."""
    verts = np.asarray(sd.verts, np.float64).reshape(-1, 3, 3)
    v0, e1, e2 = verts[:, 0], verts[:, 1] - verts[:, 0], verts[:, 2] - verts[:, 0]
    tri_mat = np.asarray(sd.tri_mat)
    sph = np.asarray(sd.spheres, np.float64)
    sph_mat = np.asarray(sd.sph_mat)
    alb = np.asarray(sd.mats["albedo"], np.float64)
    emi = np.asarray(sd.mats["emission"], np.float64)
    kinds = np.asarray(sd.mats["kind"])
    rough, ior = np.asarray(sd.mats["roughness"], np.float64), np.asarray(sd.mats["ior"], np.float64)
    cam = sd.cam
    org, fwd = np.array(cam.origin[:], np.float64), np.array(cam.forward[:], np.float64)
    right, up = np.array(cam.right[:], np.float64), np.array(cam.up[:], np.float64)
    means, errs = np.zeros((height, width, 3)), np.zeros((height, width, 3))
    for y in range(height):
        for x in range(width):
            n = n_paths
            sx = (x + rng.random(n)) * cam.scale - cam.cx
            sy = (y + rng.random(n)) * cam.scale - cam.cy
            d = fwd[None] + sx[:, None] * right[None] + sy[:, None] * up[None]
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            o = np.broadcast_to(org, d.shape).copy()
            T = np.ones((n, 3))
            L = np.zeros((n, 3))
            alive = np.ones(n, bool)
            for depth in range(1, max_depth + 1):
                idx = np.nonzero(alive)[0]
                if idx.size == 0:
                    break
                oo, dd = o[idx], d[idx]
                t_best = np.full(idx.size, np.inf)
                nrm = np.zeros((idx.size, 3))
                mat = np.zeros(idx.size, np.int64)
                for k in range(len(v0)):  # Moeller-Trumbore, no culling
                    p = np.cross(dd, e2[k])
                    det = p @ e1[k]
                    ok = np.abs(det) > 1e-14
                    inv = np.where(ok, 1.0 / np.where(ok, det, 1.0), 0.0)
                    tv = oo - v0[k]
                    u = (tv * p).sum(1) * inv
                    q = np.cross(tv, e1[k])
                    v = (dd * q).sum(1) * inv
                    t = (q @ e2[k]) * inv
                    hit = ok & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 1e-9) & (t < t_best)
                    t_best = np.where(hit, t, t_best)
                    ng = np.cross(e1[k], e2[k]); ng /= np.linalg.norm(ng)
                    nrm[hit] = ng
                    mat[hit] = tri_mat[k]
                for k in range(len(sph)):
                    oc = oo - sph[k, :3]
                    b = (oc * dd).sum(1)
                    disc = b * b - ((oc * oc).sum(1) - sph[k, 3] ** 2)
                    sq = np.sqrt(np.maximum(disc, 0.0))
                    t0, t1 = -b - sq, -b + sq
                    t = np.where(t0 > 1e-9, t0, t1)
                    hit = (disc > 0) & (t > 1e-9) & (t < t_best)
                    t_best = np.where(hit, t, t_best)
                    pn = (oo + t[:, None] * dd - sph[k, :3]) / sph[k, 3]
                    nrm[hit] = pn[hit]
                    mat[hit] = sph_mat[k]
                miss = ~np.isfinite(t_best)
                L[idx[miss]] += T[idx[miss]] * np.asarray(sd.sky, np.float64)
                alive[idx[miss]] = False
                keep = ~miss
                idx, dd, nrm, mat, t_best, oo = idx[keep], dd[keep], nrm[keep], mat[keep], t_best[keep], oo[keep]
                flip = (nrm * dd).sum(1) > 0
                nrm[flip] *= -1.0
                L[idx] += T[idx] * emi[mat]
                if depth >= max_depth:
                    alive[idx] = False
                    break
                m = idx.size
                u1, u2, u3 = rng.random(m), rng.random(m), rng.random(m)
                a = np.where(np.abs(nrm[:, 0:1]) > 0.5, np.array([[0.0, 1.0, 0.0]]), np.array([[1.0, 0.0, 0.0]]))
                tx = np.cross(a, nrm); tx /= np.linalg.norm(tx, axis=1, keepdims=True)
                ty = np.cross(nrm, tx)
                cosi = np.clip(-(dd * nrm).sum(1), 0.0, 1.0)
                kd = kinds[mat]
                wi = np.zeros((m, 3)); W = np.ones((m, 3)); side = np.ones(m); ok = np.ones(m, bool)
                # ---- Lambert: cosine-weighted direction, weight = albedo
                lam = kd == 0
                cz = u1 if drop_cosine else np.sqrt(u1)
                sz = np.sqrt(np.maximum(0.0, 1.0 - cz * cz))
                wl = (sz * np.cos(2 * np.pi * u2))[:, None] * tx + (sz * np.sin(2 * np.pi * u2))[:, None] * ty + cz[:, None] * nrm
                wi[lam] = wl[lam]; W[lam] = alb[mat][lam]
                # ---- metal: Schlick Fresnel with the albedo as F0; mirror, or GGX with the separable Smith term
                met = kd == 1
                if met.any():
                    al = rough[mat]
                    mir = met & (al == 0.0)
                    refl = dd + 2.0 * cosi[:, None] * nrm
                    wi[mir] = refl[mir]
                    W[mir] = (alb[mat] + (1.0 - alb[mat]) * ((1.0 - cosi) ** 5)[:, None])[mir]
                    rgh = met & (al > 0.0)
                    if rgh.any():
                        al2 = np.where(rgh, al, 1.0) ** 2
                        ch = np.sqrt((1.0 - u1) / (1.0 + (al2 - 1.0) * u1))  # cos(theta_h) ~ D(h) cos(theta_h)
                        sh = np.sqrt(np.maximum(0.0, 1.0 - ch * ch))
                        hv = (sh * np.cos(2 * np.pi * u2))[:, None] * tx + (sh * np.sin(2 * np.pi * u2))[:, None] * ty + ch[:, None] * nrm
                        woh = -(dd * hv).sum(1)
                        wr = 2.0 * woh[:, None] * hv + dd
                        ci = (wr * nrm).sum(1)
                        good = (woh > 0.0) & (ci > 0.0)
                        aa = np.where(rgh, al, 1.0)
                        g1o = 2.0 * cosi / (cosi + np.sqrt(aa * aa + (1.0 - aa * aa) * cosi * cosi) + 1e-300)
                        g1i = 2.0 * ci / (ci + np.sqrt(aa * aa + (1.0 - aa * aa) * ci * ci) + 1e-300)
                        fr = alb[mat] + (1.0 - alb[mat]) * ((1.0 - np.clip(woh, 0.0, 1.0)) ** 5)[:, None]
                        gg = 1.0 if wrong == "no_masking" else g1o * g1i
                        wgt = fr * (gg * woh / np.maximum(cosi * ch, 1e-300))[:, None]  # f cos_i / pdf, pdf = D cos_h / (4 wo.h)
                        wi[rgh] = wr[rgh]; W[rgh] = wgt[rgh]
                        ok &= ~(rgh & ~good)
                # ---- glass: Snell + exact unpolarised Fresnel, the lobe chosen with probability F; weight = albedo
                die = kd == 2
                if die.any():
                    n1 = np.where(flip, ior[mat], 1.0); n2 = np.where(flip, 1.0, ior[mat])  # flip: the ray is leaving the medium
                    eta = n1 / n2
                    s2 = eta * eta * (1.0 - cosi * cosi)
                    tir = s2 >= 1.0
                    ct = np.sqrt(np.maximum(0.0, 1.0 - s2))
                    rs = (n1 * cosi - n2 * ct) / (n1 * cosi + n2 * ct + 1e-300)
                    rp = (n2 * cosi - n1 * ct) / (n2 * cosi + n1 * ct + 1e-300)
                    fres = np.where(tir, 1.0, 0.5 * (rs * rs + rp * rp))
                    do_refl = (u3 < fres) if wrong != "no_reflection" else tir
                    refl = dd + 2.0 * cosi[:, None] * nrm
                    refr = eta[:, None] * dd + (eta * cosi - ct)[:, None] * nrm
                    wd = np.where(do_refl[:, None], refl, refr)
                    wi[die] = wd[die]; W[die] = alb[mat][die]
                    side[die & ~do_refl] = -1.0
                wi /= np.maximum(np.linalg.norm(wi, axis=1, keepdims=True), 1e-300)
                alive[idx[~ok]] = False
                T[idx] *= W
                if depth >= rr_start:
                    q = np.full(m, 0.85) if own_roulette else np.minimum(T[idx].max(1), 0.95)
                    survive = rng.random(m) < q
                    T[idx] /= np.where(q > 0, q, 1.0)[:, None]
                    alive[idx[~survive]] = False
                o[idx] = oo + t_best[:, None] * dd + (side * 1e-4)[:, None] * nrm
                d[idx] = wi
            means[y, x] = L.mean(0)
            errs[y, x] = L.std(0, ddof=1) / np.sqrt(n)
    return means, errs
