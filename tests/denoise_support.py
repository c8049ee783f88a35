"""TEST INFRASTRUCTURE for rtw_denoise: one seeded input, the formula of include/rtwin.h evaluated directly in NumPy (float64, or float32 for the
yardstick of the tolerance), and the gamma pack by counting thresholds.  Arrays are (H, W, channels) in the buffers' own layouts."""
import numpy as np

EPS, H5 = 1e-3, (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)
DEMODULATE, SAME_SHAPE = 1, 2
DEFAULTS = (5, 0.6, 0.3, 0.1, DEMODULATE | SAME_SHAPE)        # rtw_denoise_default_params: levels, sigma colour / normal / depth, flags


def inputs(W, H, seed=7):
    """accum (sum.xyz, int count 3), geom (sum n.xyz, sum z) and albedo (sum rgb, int count 2), ids (shape, triangle): two surfaces either side of a
    diagonal, a block of misses, noisy colour, and -- from 15 pixels on -- a firefly, a NaN, a +inf, and a pixel with each count 0"""
    r = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    far = (xx * H + yy * W) >= W * H                                   # the diagonal edge
    miss = (xx < W // 4) & (yy >= H // 2) & (yy < H // 2 + max(H // 4, 1)) & (W * H >= 15)
    n = np.where(far[..., None], (0.8, 0.0, 0.6), (0.0, 0.6, 0.8)) + 0.03 * np.sin(0.3 * xx + 0.2 * yy)[..., None]
    z = np.where(far, 9.0 + 0.03 * yy, 5.0 + 0.02 * xx)
    A = np.where(far[..., None], (0.9, 0.6, 0.0), (0.2, 0.7, 0.9)) * np.where(((xx // 3 + yy // 2) & 1)[..., None] == 1, 1.0, (0.5, 0.0, 1.0))
    shape = np.where(far, 2, 0)
    n[miss], z[miss], A[miss], shape[miss] = 0.0, 1000.0, (0.5, 0.7, 1.0), -1
    C = A * (0.2 + 0.6 * (yy / max(H - 1, 1)))[..., None] * r.uniform(0.2, 1.8, (H, W, 3))
    cfb, cf = np.full((H, W), 3, np.int32), np.full((H, W), 2, np.int32)
    if W * H >= 15:
        m, flat = W * H, C.reshape(-1, 3)
        flat[m // 3], flat[2 * m // 3, 1], flat[m - 1 - m // 7, 2] = 50.0, np.nan, np.inf
        cfb.reshape(-1)[m // 2], cf.reshape(-1)[m // 2 + 1] = 0, 0
    f32 = np.float32
    accum = np.concatenate([(C * 3).astype(f32), cfb.view(f32)[..., None]], -1) * np.where(cfb == 0, 0, 1).astype(f32)[..., None]
    geom = np.concatenate([n * 2, z[..., None] * 2], -1).astype(f32)
    albedo = np.concatenate([(A * 2).astype(f32), cf.view(f32)[..., None]], -1)
    ids = np.stack([shape, r.integers(0, 99, (H, W))], -1).astype(np.int32)
    return np.ascontiguousarray(accum), geom, np.ascontiguousarray(albedo), ids


def shifted(a, ox, oy):
    """a[y + oy, x + ox] at (y, x); zeros (False) where that lies outside"""
    H, W = a.shape[:2]
    out = np.zeros_like(a)
    if abs(ox) < W and abs(oy) < H:
        out[max(0, -oy):min(H, H - oy), max(0, -ox):min(W, W - ox)] = a[max(0, oy):min(H, H + oy), max(0, ox):min(W, W + ox)]
    return out


def reference(accum, geom, albedo, ids, params, dtype=np.float64):
    """out (H, W, 3) of include/rtwin.h's formula, every operation in `dtype`"""
    t = dtype
    levels, sc, sn, sd, flags = params
    sc, sn, sd = (t(np.float32(v)) for v in (sc, sn, sd))
    with np.errstate(all="ignore"):
        cfb, cf, shape = accum[..., 3].view(np.int32), albedo[..., 3].view(np.int32), ids[..., 0]
        empty = (cfb == 0) | (cf == 0)
        nfb, nf = np.where(empty, 1, cfb).astype(t)[..., None], np.where(empty, 1, cf).astype(t)[..., None]
        C, n, z, A = accum[..., :3].astype(t) / nfb, geom[..., :3].astype(t) / nf, geom[..., 3].astype(t) / nf[..., 0], albedo[..., :3].astype(t) / nf + t(EPS)
        bad = ~np.isfinite(C).all(-1)
        usable = ~(empty | bad)
        img = C / A if flags & DEMODULATE else C
        for i in range(levels):
            sw, acc = np.zeros(z.shape, t), np.zeros(C.shape, t)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    ox, oy = dx << i, dy << i
                    ok, iq = shifted(usable, ox, oy), shifted(img, ox, oy)
                    if flags & SAME_SHAPE:
                        ok = ok & (shifted(shape, ox, oy) == shape)
                    e = np.zeros(z.shape, t)
                    if sc > 0:
                        e = e + np.where(bad, t(0), ((img - iq) ** 2).sum(-1) / (sc * t(2.0 ** -i)) ** 2)
                    if sn > 0:
                        e = e + ((n - shifted(n, ox, oy)) ** 2).sum(-1) / sn ** 2
                    if sd > 0:
                        e = e + ((z - shifted(z, ox, oy)) / (sd * np.maximum(np.abs(z), t(1e-6)))) ** 2
                    w = np.where(ok, t(H5[dx + 2]) * t(H5[dy + 2]) * np.exp(-e), t(0))
                    sw, acc = sw + w, acc + np.where(ok[..., None], w[..., None] * iq, t(0))
            img = np.where((sw > 0)[..., None], acc / sw[..., None], np.where(bad[..., None], t(0), img))
        out = img * A if flags & DEMODULATE else img
        return np.where(empty[..., None], t(0), out)


def error(got, ref64):
    """max |got - ref64| / max(1, max |ref64| over finite pixels)"""
    return float(np.abs(got.astype(np.float64) - ref64).max() / max(1.0, np.abs(ref64[np.isfinite(ref64)]).max()))


def pack(thr, rgb):
    """the ARGB words of float32 colours (n, 3): per channel the largest k with thr[k] <= c; 0 for c <= 0 or NaN (255 for -inf), 255 for c >= 1"""
    k = np.searchsorted(thr, rgb, side="right").astype(np.int64) - 1
    k = np.where(rgb >= 1, 255, np.where(rgb > 0, np.clip(k, 0, 255), np.where(rgb == -np.inf, 255, 0))).astype(np.uint32)
    return np.uint32(255 << 24) | k[:, 0] << 16 | k[:, 1] << 8 | k[:, 2]
