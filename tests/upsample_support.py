"""TEST INFRASTRUCTURE for rtw_upsample: a low-resolution frame and features at both sizes under one camera (reproject_support's sphere over the
checkered plane before the sky), and the formula of include/rtwin.h evaluated directly in NumPy (float64, or float32 for the yardstick of the tolerance)
with, per pixel, the round that decided it and the margin of its round decisions.  Arrays are (H, W, channels) in the buffers' own layouts."""
import numpy as np

import reproject_support as RS
from denoise_support import error as _error, pack  # noqa: F401

EPS, SW_MIN, MARGIN, CAP, DEMODULATE, SAME_SHAPE = 1e-3, 1e-3, 1e-3, 0.03, 1, 2
DEFAULTS = (0.3, 0.1, DEMODULATE | SAME_SHAPE)          # rtw_upsample_default_params: sigma_normal, sigma_depth, flags
PLAIN = (0.0, 0.0, 0)                                   # every weight is its b: a pixel that lands on a low pixel returns that pixel's mean colour
K4 = (1 / 8, 3 / 8, 3 / 8, 1 / 8)
FRAMES = [(1, 1, 1, 1), (6, 4, 3, 2), (37, 23, 37, 23), (74, 46, 37, 23), (111, 69, 37, 23), (60, 36, 40, 24), (300, 36, 100, 12), (296, 184, 37, 23)]
CASES = [f + (DEFAULTS,) for f in FRAMES] + [(74, 46, 37, 23, p) for p in ((0.3, 0.1, SAME_SHAPE), (0.3, 0.1, DEMODULATE), (0.0, 0.1, 3), (0.3, 0.0, 3), (0.05, 0.01, 3))]
EMUL_CASES = [CASES[1], CASES[3], CASES[5]]


def inputs(W, H, w, h):
    """(lo, f_hi): lo = (accum, geom, albedo, ids) at w x h -- 2 passes over 3 feature passes, noisy colour with, from 15 pixels on, a firefly, a NaN
    pixel and an empty patch; f_hi = (geom, albedo, ids) at W x H after 2 feature passes with, from 15 pixels on, an empty patch of its own"""
    geom, albedo, ids, A = RS.features(w, h, RS.HOME, 3)
    C, cnt, m = A * (0.3 + RS.noise(w, h, 1)), np.full((h, w), 2, np.int32), w * h
    if m >= 15:
        C.reshape(-1, 3)[m // 3], C.reshape(-1, 3)[2 * m // 3, 1] = 50.0, np.nan
        cnt[h // 3:h // 3 + max(h // 5, 1), w // 2:w // 2 + max(w // 6, 1)] = 0
    accum = np.concatenate([(C * cnt[..., None]).astype(np.float32), cnt.view(np.float32)[..., None]], -1) * (cnt != 0).astype(np.float32)[..., None]
    hg, ha, hi, _ = RS.features(W, H, RS.HOME, 2)
    if W * H >= 15:
        hg[H // 2:H // 2 + max(H // 6, 1), W // 5:W // 5 + max(W // 7, 1)], ha[H // 2:H // 2 + max(H // 6, 1), W // 5:W // 5 + max(W // 7, 1)] = 0.0, 0.0
    return (np.ascontiguousarray(accum), geom, albedo, ids), (hg, ha, hi)


def corner(size, low, t):
    """step 1 for every pixel of one axis: (x0, tx)"""
    n = (np.arange(size) - size // 2) * low
    k = n // size
    return k + low // 2, (n - k * size).astype(t) / t(size)


def reference(lo, f_hi, params, dtype=np.float64):
    """(out (H, W, 3) in `dtype`, count (H, W), round (H, W): 0 for an empty pixel, else the round that decided it, margin (H, W):
    |sw - SW_MIN| / SW_MIN of each round decision taken): include/rtwin.h's formula with every operation in `dtype`"""
    t = dtype
    sn, sd, flags, swmin = t(np.float32(params[0])), t(np.float32(params[1])), params[2], t(np.float32(SW_MIN))
    (h, w), (H, W) = lo[0].shape[:2], f_hi[0].shape[:2]
    with np.errstate(all="ignore"):
        cfb, cf, cp = lo[0][..., 3].view(np.int32), lo[2][..., 3].view(np.int32), f_hi[1][..., 3].view(np.int32)
        le, pe = (cfb == 0) | (cf == 0), cp == 0
        nfb, nf, nfp = (np.where(e, 1, c).astype(t)[..., None] for e, c in ((le, cfb), (le, cf), (pe, cp)))
        C = lo[0][..., :3].astype(t) / nfb
        lI = C / (lo[2][..., :3].astype(t) / nf + t(EPS)) if flags & DEMODULATE else C
        lu, ln, lz, ls = ~le & np.isfinite(C).all(-1), lo[1][..., :3].astype(t) / nf, lo[1][..., 3].astype(t) / nf[..., 0], lo[3][..., 0] & 0x3FFFFFFF
        n, z, M, s = f_hi[0][..., :3].astype(t) / nfp, f_hi[0][..., 3].astype(t) / nfp[..., 0], f_hi[1][..., :3].astype(t) / nfp + t(EPS), f_hi[2][..., 0] & 0x3FFFFFFF
        (x0, tx), (y0, ty) = corner(W, w, t), corner(H, h, t)
        x0, y0, tx, ty = np.broadcast_to(x0, (H, W)), np.broadcast_to(y0[:, None], (H, W)), np.broadcast_to(tx, (H, W)), np.broadcast_to(ty[:, None], (H, W))

        def taps(offsets, weights):
            sw, sc = np.zeros((H, W), t), np.zeros((H, W, 3), t)
            for (dx, dy), b in zip(offsets, weights):
                qx, qy = x0 + dx, y0 + dy
                q = (np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1))
                ok = (b != 0) & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h) & lu[q] & ((ls[q] == s) if flags & SAME_SHAPE else True)
                e = np.zeros((H, W), t)
                if sn > 0:
                    e = e + ((n - ln[q]) ** 2).sum(-1) / sn ** 2
                if sd > 0:
                    e = e + ((z - lz[q]) / (sd * np.maximum(np.abs(z), t(1e-6)))) ** 2
                wt = np.where(ok, b * np.exp(-e), t(0))
                sw, sc = sw + wt, sc + np.where(ok[..., None], wt[..., None] * lI[q], t(0))
            return sw, sc / np.where(sw > 0, sw, t(1))[..., None]
        four = [(0, 0), (1, 0), (0, 1), (1, 1)]
        bs = [(tx if dx else t(1) - tx) * (ty if dy else t(1) - ty) for dx, dy in four]
        sw1, I1 = taps(four, bs)
        sw2, I2 = taps([(dx, dy) for dy in range(-1, 3) for dx in range(-1, 3)], [t(K4[dx + 1]) * t(K4[dy + 1]) for dy in range(-1, 3) for dx in range(-1, 3)])
        best, I3 = np.full((H, W), t(-1)), np.zeros((H, W, 3), t)
        for (dx, dy), b in zip(four, bs):
            qx, qy = x0 + dx, y0 + dy
            q = (np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1))
            better = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h) & lu[q] & (b > best)
            best, I3 = np.where(better, b, best), np.where(better[..., None], lI[q], I3)
        a1, a2 = sw1 >= swmin, sw2 >= swmin
        I = np.where(a1[..., None], I1, np.where(a2[..., None], I2, I3))
        count = np.where(pe | ~(a1 | a2 | (best >= 0)), 0, 1)
        out = np.where((count == 0)[..., None], t(0), I * M if flags & DEMODULATE else I)
        margin = np.where(pe, np.inf, np.minimum(np.abs(sw1 - swmin), np.where(a1, np.inf, np.abs(sw2 - swmin))) / swmin)
        return out, count, np.where(pe, 0, np.where(a1, 1, np.where(a2, 2, 3))), margin


def compared(rounds, margin):
    """(the pixels whose value is compared, the share of the non-empty pixels left out because a round decision fell within MARGIN of SW_MIN)"""
    keep = ~(margin < MARGIN)
    return keep, float(((rounds > 0) & ~keep).sum()) / max(int((rounds > 0).sum()), 1)


def error(got, ref64, keep):
    """denoise_support.error over the compared pixels"""
    return _error(got[keep], ref64[keep])
