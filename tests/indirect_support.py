"""Shared by the indirect-light tests (a NumPy model over the oracle; no test in here).

rtw_render_indirect (include/rtwin.h) in float32, every operation rounded on its own, from occlusion_support, lighting_support.job at (O2, m) and the
oracle's trace_closest and ray_trace(rays, keys, 1, True, ...) as in features_support.model: its paths restart at counter 0, so the scenes hold no Blend."""
import numpy as np

from camera_support import rand31
from denoise_support import pack
from lighting_support import job
from occlusion_support import STREAM, TABLE, dot3, origins, table_entries

f32 = np.float32
ALBEDO, MIRROR = 1, 2


def model(R, osc, feats, cam, W, H, lights, bias, samples, flags, first_pass, n_passes, seed, thr, into=None):
    """(accum (n, 4) with the count as a float, argb (n,), seen) after one call on top of `into` = (accum, argb) (default: a cleared framebuffer);
    seen = (a gather miss, a gather hit that is lit, a gather hit whose shadow ray is occluded, a light job culled at the gather hit)"""
    geom, albedo, ids = feats
    state, O, nrm = origins(geom, albedo, ids, cam, W, H, bias)
    accum, argb = (np.zeros((W * H, 4), f32), np.zeros(W * H, np.uint32)) if into is None else (into[0].copy(), into[1].copy())
    cast, live_px, cam = np.flatnonzero(state == 2), state != 0, np.asarray(cam, f32)
    o, n, nc = O[cast], nrm[cast], len(cast)
    dx = -(cast % W - W // 2).astype(f32) / f32(W * 2) * (f32(W) / f32(H))      # w: the unit direction of the casting pixels' pinhole rays (reproject_point's)
    dy = -(cast // W - H // 2).astype(f32) / f32(H * 2)
    w = np.stack([((cam[3 + k] * dx + cam[6 + k] * dy).astype(f32) + cam[9 + k] * cam[12]).astype(f32) for k in range(3)], 1)
    w = (w * (f32(1.0) / np.sqrt(dot3(w, w))).astype(f32)[:, None]).astype(f32)
    with np.errstate(all="ignore"):
        alb = (albedo[:, 0:3] / albedo[:, 3:4]).astype(f32) if flags & ALBEDO else np.ones((W * H, 3), f32)
    seen = np.zeros(4, bool)
    for k in range(first_pass, first_pass + n_passes):
        A, Wt = np.zeros((nc, 3), f32), np.zeros(nc, f32)
        for s in range(samples):
            v = w if flags & MIRROR else table_entries(R, rand31(seed, cast, (k * 64 + s) | STREAM, 0).astype(np.int64) % TABLE)
            dt = dot3(v, n)
            refl = (v - ((n * f32(2.0)).astype(f32) * dt[:, None]).astype(f32)).astype(f32)
            d = refl if flags & MIRROR else np.where((dt > 0)[:, None], v, refl)
            c = dot3(n, d)
            ray = (c > 0) if flags & MIRROR else np.ones(nc, bool)
            c = np.where(ray, c, f32(0))
            rays = np.concatenate([o, d, np.full((nc, 1), 1000.0, f32)], 1).astype(f32)
            hits, shape, _ = osc.trace_closest(rays)
            keys = np.stack([cast, np.full(nc, (k * 64 + s) | STREAM)], 1).astype(np.uint32)
            L = osc.ray_trace(rays, keys, 1, True, seed, W, H)              # a hit: a_s; a miss: the sky colour of d
            hit, m = ray & (shape >= 0), hits[:, 3:6]
            O2 = (hits[:, 0:3] + (m * f32(bias)).astype(f32)).astype(f32)
            E = np.zeros((nc, 3), f32)
            for j, light in enumerate(lights):
                live, srays, t = job(R, light, seed, cast, k, s, j, O2, m)
                live &= hit
                occluded = np.zeros(nc, bool)
                occluded[live] = osc.trace_closest(srays[live])[1] >= 0
                E = (E + (np.asarray(light[3], f32)[None, :] * np.where(live & ~occluded, t, f32(0))[:, None]).astype(f32)).astype(f32)
                seen[1:] |= [(live & ~occluded).any(), occluded.any(), (hit & ~live).any()]
            seen[0] |= (ray & (shape < 0)).any()
            L = np.where(hit[:, None], (L * E).astype(f32), np.where(ray[:, None], L, f32(0)))
            A, Wt = (A + (L * c[:, None]).astype(f32)).astype(f32), (Wt + c).astype(f32)
        e = np.zeros((W * H, 3), f32)
        with np.errstate(all="ignore"):
            e[cast] = (np.where((Wt > 0)[:, None], (A / Wt[:, None]).astype(f32), f32(0)) * alb[cast]).astype(f32)
        accum[live_px, 0:3] = (accum[live_px, 0:3] + e[live_px]).astype(f32)
        accum[live_px, 3] += f32(1)
    argb[live_px] = pack(thr, (accum[live_px, 0:3] / accum[live_px, 3:4]).astype(f32))
    return accum, argb, tuple(bool(b) for b in seen)
