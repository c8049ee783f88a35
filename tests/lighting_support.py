"""Shared by the lighting tests (a NumPy model over the oracle; no test in here).

rtw_render_lighting (include/rtwin.h) in float32, every product and every sum rounded on its own: a feature read-back, a camera's 13 floats, the lights
-- (type, flags, v, color, radius) tuples -- the parameters, the passes and a seed become the framebuffer (sum, count) after the call.  Pixel states and
origins are occlusion_support's, occlusion bits come from the CPU oracle (Scene.trace_closest, shape >= 0), table entries from the library."""
import numpy as np

from camera_support import rand31
from denoise_support import pack
from occlusion_support import TABLE, dot3, origins, table_entries

f32 = np.float32
STREAM, POINT, DIRECTIONAL, INVERSE_SQUARE, ALBEDO = 0xC0000000, 0, 1, 1, 1


def job(R, light, seed, pix, k, s, j, o, n):
    """steps 2 to 5 for the casting pixels `pix`: (live (n,), rays (n, 7), t (n,) = c * att where live, else 0)"""
    typ, flags, v, _, radius = light
    u = np.zeros((len(pix), 3), f32)
    if radius != 0:
        u = table_entries(R, rand31(seed, pix, (k * 64 + s) | STREAM, j).astype(np.int64) % TABLE)
    with np.errstate(all="ignore"):
        D = (np.asarray(v, f32)[None, :] + (u * f32(radius)).astype(f32)).astype(f32)
        if typ == POINT:
            D = (D - o).astype(f32)
        ln = np.sqrt(dot3(D, D)).astype(f32)
        d = (D * (f32(1.0) / ln).astype(f32)[:, None]).astype(f32)
        att = (f32(1.0) / (ln * ln).astype(f32)).astype(f32) if flags & INVERSE_SQUARE else np.ones(len(pix), f32)
        c = dot3(n, d)
        live = c > 0
        if typ == POINT:
            live &= np.isfinite(ln) & (ln > 0)
        t = np.where(live, (c * att).astype(f32), f32(0))
    dist = ln if typ == POINT else np.full(len(pix), 1000.0, f32)
    return live, np.concatenate([o, d, dist[:, None]], 1).astype(f32), t


def model(R, oracle_scene, feats, cam, W, H, lights, bias, samples, flags, first_pass, n_passes, seed, thr, into=None):
    """(accum (n, 4) with the count as a float, argb (n,), seen) after one call on top of `into` = (accum, argb) (default: a cleared framebuffer);
    seen = (a job was lit, a live job was occluded, a job was culled)"""
    geom, albedo, ids = feats
    state, O, nrm = origins(geom, albedo, ids, cam, W, H, bias)
    accum = np.zeros((W * H, 4), f32) if into is None else into[0].copy()
    argb = np.zeros(W * H, np.uint32) if into is None else into[1].copy()
    cast = np.flatnonzero(state == 2)
    o, n = O[cast], nrm[cast]
    with np.errstate(all="ignore"):
        alb = (albedo[:, 0:3] / albedo[:, 3:4]).astype(f32)
    seen = [False, False, False]
    live_px = state != 0
    for k in range(first_pass, first_pass + n_passes):
        e = np.ones((W * H, 3), f32)
        ec = np.zeros((len(cast), 3), f32)
        for j, light in enumerate(lights):
            total = np.zeros(len(cast), f32)
            for s in range(samples):
                live, rays, t = job(R, light, seed, cast, k, s, j, o, n)
                occluded = np.zeros(len(cast), bool)
                occluded[live] = oracle_scene.trace_closest(rays[live])[1] >= 0
                total = (total + np.where(occluded, f32(0), t)).astype(f32)
                seen = [seen[0] or bool((live & ~occluded).any()), seen[1] or bool(occluded.any()), seen[2] or bool((~live).any())]
            vis = (total / f32(samples)).astype(f32)
            ec = (ec + (np.asarray(light[3], f32)[None, :] * vis[:, None]).astype(f32)).astype(f32)
        e[cast] = ec
        if flags & ALBEDO:
            e = (e * alb).astype(f32)
        accum[live_px, 0:3] = (accum[live_px, 0:3] + e[live_px]).astype(f32)
        accum[live_px, 3] += f32(1)
    argb[live_px] = pack(thr, (accum[live_px, 0:3] / accum[live_px, 3:4]).astype(f32))
    return accum, argb, tuple(seen)
