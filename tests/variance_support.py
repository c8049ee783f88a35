"""TEST INFRASTRUCTURE for rtw_denoise_variance and rtw_reproject_moments: inputs with uneven history lengths and luminance moments, and the formulas of
include/rtwin.h evaluated directly in NumPy (float64, or float32 for the yardstick of the tolerances).  Builds on denoise_support and reproject_support;
arrays are (H, W, channels) in the buffers' own layouts."""
import numpy as np

import reproject_support as RS
from denoise_support import DEMODULATE, EPS, H5, SAME_SHAPE, error, pack, shifted  # noqa: F401
from denoise_support import inputs as base_inputs

DEFAULTS = (5, 4.0, 0.3, 0.1, DEMODULATE | SAME_SHAPE, 4)        # rtw_denoise_variance_default_params: levels, sigma lum / normal / depth, flags, min_history
K3 = (1 / 4, 1 / 2, 1 / 4)
LENGTHS = np.array([1, 2, 3, 4, 9, 32], np.int32)
D, FRAMES = DEFAULTS, [(1, 1), (5, 3), (37, 23), (131, 70), (300, 33)]
PARAMS = [(1,) + D[1:], (6,) + D[1:], D[:5] + (1,), D[:5] + (64,), D[:4] + (DEMODULATE, 4), D[:4] + (SAME_SHAPE, 4), (5, 4.0, 0, 0) + D[4:]]
CASES, EMUL_FRAMES = [(W, H, D) for W, H in FRAMES] + [(37, 23, p) for p in PARAMS], FRAMES[1:4]
# 8 x the largest error of the float32 NumPy evaluation against the float64 one: of reference over CASES (6.296e-07, 131x70), of moments_reference
# over reproject_support.CASES (1.183e-07, 131x70 roll) -- profiles/variance_experiments.md section 1
BOUND, BOUND_MOMENTS = 5.037e-06, 9.462e-07


def lum(v, t):
    return (t(np.float32(0.2126)) * v[..., 0] + t(np.float32(0.7152)) * v[..., 1]) + t(np.float32(0.0722)) * v[..., 2]


def inputs(W, H):
    """denoise_support's frame with history lengths N from LENGTHS by a fixed hash (the sums rescaled to match), and moments (H, W, 2): mu1 near
    lum(I_0), mu2 = mu1^2 (1 + u) with u in [0.05, 1]; a patch with mu2 == mu1^2 exactly (mu1 a multiple of 1/64), one with mu2 < mu1^2"""
    accum, geom, albedo, ids = base_inputs(W, H)
    f32 = np.float32
    with np.errstate(all="ignore"):
        cfb = accum[..., 3].view(np.int32)
        n = np.where(cfb == 0, 0, LENGTHS[(RS.noise(W, H, 5)[..., 0] * 6).astype(np.int64)]).astype(np.int32)
        C = accum[..., :3] / f32(3)
        accum = np.ascontiguousarray(np.concatenate([np.where((n == 0)[..., None], f32(0), C * n[..., None].astype(f32)), n.view(f32)[..., None]], -1).astype(f32))
        I0 = C.astype(np.float64) / (albedo[..., :3].astype(np.float64) / 2 + EPS)
        l = lum(I0, np.float64)
    u = RS.noise(W, H, 6)
    mu1 = np.minimum(np.where(np.isfinite(l) & (n > 0), l, 0.5) * (0.9 + 0.2 * u[..., 0]), 60.0).astype(f32)
    mu2 = (mu1.astype(np.float64) ** 2 * (1.05 + 0.95 * u[..., 1])).astype(f32)
    exact, below = (slice(H // 4, H // 2), slice(W // 2, 3 * W // 4)), (slice(H // 2, 3 * H // 4), slice(W // 2, 3 * W // 4))
    mu1[exact] = np.round(mu1[exact] * 64) / 64
    mu2[exact], mu2[below] = mu1[exact] * mu1[exact], mu1[below] * mu1[below] * f32(0.9)
    return accum, geom, albedo, ids, np.ascontiguousarray(np.stack([mu1, mu2], -1))


def reference(accum, geom, albedo, ids, mu, params, dtype=np.float64):
    """out (H, W, 3) of include/rtwin.h's formula for rtw_denoise_variance, every operation in `dtype`"""
    t = dtype
    levels, sl, sn, sd, flags, minh = params
    sl, sn, sd = (t(np.float32(v)) for v in (sl, sn, sd))
    with np.errstate(all="ignore"):
        cfb, cf, shape = accum[..., 3].view(np.int32), albedo[..., 3].view(np.int32), ids[..., 0]
        empty = (cfb == 0) | (cf == 0)
        nfb, nf = np.where(empty, 1, cfb).astype(t)[..., None], np.where(empty, 1, cf).astype(t)[..., None]
        C, n, z, A = accum[..., :3].astype(t) / nfb, geom[..., :3].astype(t) / nf, geom[..., 3].astype(t) / nf[..., 0], albedo[..., :3].astype(t) / nf + t(EPS)
        bad = ~np.isfinite(C).all(-1)
        usable = ~(empty | bad)
        img = C / A if flags & DEMODULATE else C
        m1, m2 = mu[..., 0].astype(t), mu[..., 1].astype(t)

        def taken(ox, oy, same_shape):
            ok = shifted(usable, ox, oy)
            return ok & (shifted(shape, ox, oy) == shape) if same_shape else ok

        def guided(e, ox, oy):
            if sn > 0:
                e = e + ((n - shifted(n, ox, oy)) ** 2).sum(-1) / sn ** 2
            if sd > 0:
                e = e + ((z - shifted(z, ox, oy)) / (sd * np.maximum(np.abs(z), t(1e-6)))) ** 2
            return e

        s0, s1, s2 = np.zeros(z.shape, t), np.zeros(z.shape, t), np.zeros(z.shape, t)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                w = np.where(taken(dx, dy, flags & SAME_SHAPE), np.exp(-guided(np.zeros(z.shape, t), dx, dy)), t(0))
                s0, s1, s2 = s0 + w, s1 + w * shifted(m1, dx, dy), s2 + w * shifted(m2, dx, dy)
        d0 = np.where(s0 > 0, s0, t(1))
        spatial = np.where(s0 > 0, np.maximum(s2 / d0 - (s1 / d0) * (s1 / d0), t(0)) * (t(minh) / nfb[..., 0]), t(0))
        V = np.where(empty, t(0), np.where(cfb >= minh, np.maximum(m2 - m1 * m1, t(0)), spatial))
        for i in range(levels):
            sk, sg = np.zeros(z.shape, t), np.zeros(z.shape, t)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    ok, k = taken(dx, dy, False), t(K3[dx + 1]) * t(K3[dy + 1])
                    sk, sg = sk + np.where(ok, k, t(0)), sg + np.where(ok, k * shifted(V, dx, dy), t(0))
            g = np.where(sk > 0, sg / np.where(sk > 0, sk, t(1)), t(0))
            l = lum(img, t)
            sw, acc, sv = np.zeros(z.shape, t), np.zeros(C.shape, t), np.zeros(z.shape, t)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    ox, oy = dx << i, dy << i
                    ok, iq = taken(ox, oy, flags & SAME_SHAPE), shifted(img, ox, oy)
                    e = np.zeros(z.shape, t)
                    if sl > 0:
                        e = e + np.where(bad, t(0), np.abs(l - shifted(l, ox, oy)) / (sl * np.sqrt(g) + t(np.float32(1e-4))))
                    w = np.where(ok, t(H5[dx + 2]) * t(H5[dy + 2]) * np.exp(-guided(e, ox, oy)), t(0))
                    sw, acc, sv = sw + w, acc + np.where(ok[..., None], w[..., None] * iq, t(0)), sv + np.where(ok, (w * w) * shifted(V, ox, oy), t(0))
            img = np.where((sw > 0)[..., None], acc / sw[..., None], np.where(bad[..., None], t(0), img))
            V = np.where(sw > 0, sv / (sw * sw), V)
        out = img * A if flags & DEMODULATE else img
        return np.where(empty[..., None], t(0), out)


def history_moments(hist, salt=11):
    """moments (H, W, 2) for a history frame of reproject_support.inputs: multiples of 1/256, so that their products with the history lengths are exact"""
    H, W = hist[0].shape[:2]
    u = RS.noise(W, H, salt)
    mu1 = np.round((0.2 + 0.8 * u[..., 0]) * 256) / 256
    mu2 = np.round(mu1 * mu1 * (1.05 + 0.95 * u[..., 1]) * 256) / 256
    return np.ascontiguousarray(np.stack([mu1, mu2], -1).astype(np.float32))


def moments_reference(cam_cur, cam_prev, cur, hist, m_hist, params, moments_history, dtype=np.float64):
    """(mu (H, W, 2) in `dtype`, N, margin): reproject_support.reference over the two-channel frames -- the current one (l, l * l) of I_cur with count 1,
    the history m_hist with the history's counts -- without demodulation and with moments_history in max_history's place"""
    t = dtype
    accum, geom, albedo, ids = cur
    with np.errstate(all="ignore"):
        cfb, cf = accum[..., 3].view(np.int32), albedo[..., 3].view(np.int32)
        empty = (cfb == 0) | (cf == 0)
        nfb, nf = np.where(empty, 1, cfb).astype(t)[..., None], np.where(empty, 1, cf).astype(t)[..., None]
        I = accum[..., :3].astype(t) / nfb
        if params[3] & RS.DEMODULATE:
            I = I / (albedo[..., :3].astype(t) / nf + t(EPS))
        l = lum(I, t)
        one = np.where(empty, 0, 1).astype(np.int32)
        s_cur = np.ascontiguousarray(np.stack([l, l * l, np.zeros_like(l), one.view(np.float32)], -1).astype(np.float32))
        hcnt = hist[0][..., 3].view(np.int32)
        s_hist = np.ascontiguousarray(np.concatenate([m_hist * hcnt[..., None].astype(np.float32), np.zeros_like(m_hist[..., :1]), hcnt.view(np.float32)[..., None]], -1))
        total, n, margin = RS.reference(cam_cur, cam_prev, (s_cur, geom, albedo, ids), (s_hist,) + tuple(hist[1:]), (params[0], params[1], moments_history, 0), dtype)
        return (total / np.maximum(n, 1).astype(t)[..., None])[..., :2], n, margin


def moments_error(got, ref, compared):
    """reproject_support.error's measure on the moments: max |got - ref64| / max(1, max |ref64|) over the compared pixels"""
    return float(np.abs(got[compared].astype(np.float64) - ref[compared]).max() / max(1.0, np.abs(ref[compared]).max())) if compared.any() else 0.0
