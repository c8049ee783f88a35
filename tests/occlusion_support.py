"""Shared by the occlusion tests (a NumPy model over the oracle; no test in here).

rtw_render_occlusion (include/rtwin.h) in float32, every product and every sum rounded on its own: a feature read-back (geom, albedo, ids -- the
counts as floats, as FeatureBuffers.read gives them), a camera's 13 floats, the parameters, the passes and a seed become the per-pixel rays and
weights and the framebuffer (sum, count) after the call.  Occlusion bits come from the CPU oracle (Scene.trace_closest, shape >= 0), table entries
from the library's rtw_unit_table_entry."""
import numpy as np

from camera_support import rand31
from denoise_support import pack

f32 = np.float32
STREAM, TABLE, COSINE = 0x40000000, 0xFFFFFF, 1


def dot3(a, b):
    return ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]).astype(f32) + a[:, 2] * b[:, 2]).astype(f32)


def origins(geom, albedo, ids, cam, W, H, bias):
    """(state (n,): 0 EMPTY, 1 OPEN, 2 CAST;  O (n, 3);  n (n, 3)) -- steps 1 to 3; O and n are zero where the pixel does not cast"""
    cam = np.asarray(cam, f32)
    eye, right, up, fwd, focal = cam[0:3], cam[3:6], cam[6:9], cam[9:12], cam[12]
    cf = albedo[:, 3].astype(f32)
    with np.errstate(all="ignore"):
        m = (geom[:, 0:3] / cf[:, None]).astype(f32)
        z = (geom[:, 3] / cf).astype(f32)
        sq = dot3(m, m)
        nrm = (m * (f32(1.0) / np.sqrt(sq)).astype(f32)[:, None]).astype(f32)
    state = np.where(cf == 0, 0, np.where((ids[:, 0] < 0) | (np.abs(sq) < np.finfo(f32).eps), 1, 2))
    pix = np.arange(W * H, dtype=np.int64)
    x, y = pix % W, pix // W
    dx = -(x - W // 2).astype(f32) / f32(W * 2) * (f32(W) / f32(H))
    dy = -(y - H // 2).astype(f32) / f32(H * 2)
    v = np.stack([((right[k] * dx + up[k] * dy).astype(f32) + fwd[k] * focal).astype(f32) for k in range(3)], 1)
    inv = (f32(1.0) / np.sqrt(dot3(v, v))).astype(f32)
    with np.errstate(all="ignore"):
        P = (eye[None, :] + ((v * inv[:, None]).astype(f32) * z[:, None]).astype(f32)).astype(f32)
        O = (P + (nrm * f32(bias)).astype(f32)).astype(f32)
    cast = (state == 2)[:, None]
    return state, np.where(cast, O, f32(0)).astype(f32), np.where(cast, nrm, f32(0)).astype(f32)


_table = {}


def table_entries(R, idx):
    out = np.empty((len(idx), 3), f32)
    for j, i in enumerate(idx.tolist()):
        if i not in _table:
            _table[i] = R.api.unit_table_entry(i)
        out[j] = _table[i]
    return out


def model(R, oracle_scene, feats, cam, W, H, radius, bias, samples, flags, first_pass, n_passes, seed, thr, into=None):
    """(accum (n, 4) with the count as a float, argb (n,)) after one call on top of `into` = (accum, argb) (default: a cleared framebuffer)"""
    geom, albedo, ids = feats
    state, O, nrm = origins(geom, albedo, ids, cam, W, H, bias)
    accum = np.zeros((W * H, 4), f32) if into is None else into[0].copy()
    argb = np.zeros(W * H, np.uint32) if into is None else into[1].copy()
    cast = np.flatnonzero(state == 2)
    o, n = O[cast], nrm[cast]
    for k in range(first_pass, first_pass + n_passes):
        a = np.ones(W * H, f32)
        A, Wt = np.zeros(len(cast), f32), np.zeros(len(cast), f32)
        for s in range(samples):
            idx = (rand31(seed, cast, (k * 64 + s) | STREAM, 0).astype(np.int64) % TABLE)
            v = table_entries(R, idx)
            dt = dot3(v, n)
            refl = (v - ((n * f32(2.0)).astype(f32) * dt[:, None]).astype(f32)).astype(f32)
            d = np.where((dt > 0)[:, None], v, refl)
            rays = np.concatenate([o, d, np.full((len(cast), 1), radius, f32)], 1).astype(f32)
            occluded = oracle_scene.trace_closest(rays)[1] >= 0
            nd = dot3(n, d)
            c = np.where(nd > 0, nd, f32(0)) if flags & COSINE else np.ones(len(cast), f32)
            A = (A + np.where(occluded, f32(0), c)).astype(f32)
            Wt = (Wt + c).astype(f32)
        with np.errstate(all="ignore"):
            a[cast] = np.where(Wt > 0, (A / Wt).astype(f32), f32(1))
        live = state != 0
        accum[live, 0:3] = (accum[live, 0:3] + a[live, None]).astype(f32)
        accum[live, 3] += f32(1)
    live = state != 0
    argb[live] = pack(thr, (accum[live, 0:3] / accum[live, 3:4]).astype(f32))
    return accum, argb
