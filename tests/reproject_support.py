"""TEST INFRASTRUCTURE for rtw_reproject: cameras, a deterministic pair of frames over a tiny analytic scene, and the formula of include/rtwin.h
evaluated directly in NumPy (float64, or float32 for the yardstick of the tolerance) with, per pixel, the margin by which its decisions were taken.
Arrays are (H, W, channels) in the buffers' own layouts; a camera is its 13 floats (eye, right, up, forward, focal)."""
import numpy as np

from denoise_support import pack  # noqa: F401  (the gamma pack by counting thresholds)

EPS, SNAP, DEMODULATE, MARGIN = 1e-3, 1 / 64, 1, 1e-3
DEFAULTS = (0.05, 0.9, 32, DEMODULATE)          # rtw_reproject_default_params: depth_tolerance, normal_cos, max_history, flags
FRAMES = [(1, 1), (5, 3), (37, 23), (131, 70), (300, 33)]
PARAMS = [DEFAULTS, (0.05, 0.9, 32, 0), (0.0, 0.9, 32, DEMODULATE), (0.05, -1.0, 32, DEMODULATE), (0.05, 0.9, 1, DEMODULATE)]
EXACT = (0.0, -1.0, 32, 0)                      # identical cameras: one tap of weight 1, nothing to tolerate


def look_at(eye, target, roll_degrees=0.0, up=(0.0, 1.0, 0.0), vfov_degrees=53.13010235415598):
    """rtw_camera_look_at's basis (right = forward x up, up = right x forward), rolled about the view axis"""
    eye, f = np.asarray(eye, np.float64), np.asarray(target, np.float64) - np.asarray(eye, np.float64)
    f /= np.linalg.norm(f)
    r = np.cross(f, up)
    r /= np.linalg.norm(r)
    u, a = np.cross(r, f), np.radians(roll_degrees)
    r, u = r * np.cos(a) + u * np.sin(a), u * np.cos(a) - r * np.sin(a)
    return np.concatenate([eye, r, u, f, [0.25 / np.tan(np.radians(vfov_degrees) / 2)]]).astype(np.float32)


EYE, TARGET = np.array((0.3, 4.0, 3.5)), np.array((0.0, -0.2, 0.0))
HOME = look_at(EYE, TARGET)


def moved(right=0.0, forward=0.0, roll_degrees=0.0):
    """HOME moved along its own right and forward axes and rolled about its view axis"""
    off = right * HOME[3:6].astype(np.float64) + forward * HOME[9:12].astype(np.float64)
    return look_at(EYE + off, TARGET + off, roll_degrees)


PAIRS = {       # name: (current camera, previous camera, the history is cleared)
    "same": (HOME, HOME, False),
    "step": (HOME, moved(right=0.8), False),            # sideways: a disocclusion band beside the sphere
    "dolly": (HOME, moved(forward=-0.5), False),
    "roll": (HOME, moved(roll_degrees=40.0), False),    # about the view axis: a tile's taps spread over a box too large to stage
    "away": (HOME, look_at(EYE, 2 * EYE - TARGET), False),     # t <= 0 everywhere
    "cleared": (HOME, moved(right=0.8), True),
}
# the two smallest frames take the pairs under which no pixel of theirs decides within MARGIN (one pixel of 15 is more than the cap)
CASES = [(1, 1, "dolly", DEFAULTS), (5, 3, "roll", DEFAULTS), (300, 33, "step", DEFAULTS)] + [(W, H, k, DEFAULTS) for W, H in FRAMES[2:4] for k in PAIRS] \
    + [(37, 23, "step", p) for p in PARAMS[1:]]
EMUL_CASES = [(W, H, k, DEFAULTS) for W, H in FRAMES[2:] for k in ("step", "dolly", "roll")]


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def noise(W, H, salt):
    """a fixed hash of (x, y, channel, salt) in [0, 1)"""
    yy, xx, cc = np.mgrid[0:H, 0:W, 0:3].astype(np.uint64)
    h = (xx * 73856093 ^ yy * 19349663 ^ cc * 83492791 ^ np.uint64(salt * 2654435761)) & np.uint64(0xFFFFFFFF)
    h = (h ^ (h >> np.uint64(15))) * np.uint64(0x2C1B3C6D) & np.uint64(0xFFFFFFFF)
    return ((h ^ (h >> np.uint64(12))) & np.uint64(0xFFFF)).astype(np.float64) / 65536.0


def features(W, H, cam, count):
    """geom, albedo, ids and the albedo (H, W, 3) of a unit sphere at the origin (id 1) over the plane y = -1 (id 0) before the sky (id -1), as
    rtw_render_features lays them out after `count` passes"""
    c = cam.astype(np.float64)
    yy, xx = np.mgrid[0:H, 0:W]
    a, b = -(xx - W // 2) / (2 * W) * (W / H), -(yy - H // 2) / (2 * H)
    v = c[3:6] * a[..., None] + c[6:9] * b[..., None] + c[9:12] * c[12]
    d = v / np.linalg.norm(v, axis=-1, keepdims=True)
    with np.errstate(all="ignore"):
        bq, cq = d @ c[0:3], c[0:3] @ c[0:3] - 1.0
        ts = np.where(bq * bq - cq > 0, -bq - np.sqrt(np.abs(bq * bq - cq)), np.inf)
        ts = np.where(ts > 0, ts, np.inf)
        tp = np.where(d[..., 1] < 0, (-1.0 - c[1]) / d[..., 1], np.inf)
    z = np.minimum(np.minimum(ts, tp), 1000.0)
    P = c[0:3] + d * z[..., None]
    sphere, plane = (ts <= tp) & (ts < 1000.0), (tp < ts) & (tp < 1000.0)
    n = np.where(sphere[..., None], P, np.where(plane[..., None], (0.0, 1.0, 0.0), 0.0))
    check = ((np.floor(P[..., 0]) + np.floor(P[..., 2])).astype(np.int64) & 1) == 1
    A = np.where(sphere[..., None], (0.8, 0.3, 0.2), np.where(plane[..., None], np.where(check[..., None], (0.9, 0.9, 0.9), (0.2, 0.2, 0.6)), (0.5, 0.7, 1.0)))
    shape = np.where(sphere, 1, np.where(plane, 0, -1))
    cf = np.full((H, W), count, np.int32)
    geom = (np.concatenate([n, z[..., None]], -1) * count).astype(np.float32)
    albedo = np.ascontiguousarray(np.concatenate([(A * count).astype(np.float32), cf.view(np.float32)[..., None]], -1))
    return geom, albedo, np.stack([shape, np.zeros_like(shape)], -1).astype(np.int32), A


def inputs(W, H, cam_cur, cam_prev, cleared=False):
    """(cur, hist), each (accum, geom, albedo, ids).  cur: 2 passes over 3 feature passes, noisy colour with -- from 15 pixels on -- a firefly (50) and a
    NaN pixel; hist: 2 feature passes, history lengths 0..40 by hash with an empty patch (all 0 when cleared)"""
    out, m = [], W * H
    for k, (cam, cf) in enumerate(((cam_cur, 3), (cam_prev, 2))):
        geom, albedo, ids, A = features(W, H, cam, cf)
        C = A * (0.3 + noise(W, H, k + 1))
        cnt = np.full((H, W), 2, np.int32)
        if k == 1:
            cnt = (noise(W, H, 9)[..., 0] * 41).astype(np.int32)
            cnt[H // 3:H // 3 + max(H // 5, 1), W // 2:W // 2 + max(W // 6, 1)] = 0 if m >= 15 else cnt[0, 0]
            cnt[...] = 0 if cleared else cnt
        elif m >= 15:
            C.reshape(-1, 3)[m // 3], C.reshape(-1, 3)[2 * m // 3, 1] = 50.0, np.nan
        accum = np.concatenate([(C * cnt[..., None]).astype(np.float32), cnt.view(np.float32)[..., None]], -1) * (cnt != 0).astype(np.float32)[..., None]
        out.append((np.ascontiguousarray(accum), geom, albedo, ids))
    return out


def reference(cam_cur, cam_prev, cur, hist, params, dtype=np.float64):
    """(sum (H, W, 3) in `dtype`, N (H, W) int, margin (H, W)): include/rtwin.h's formula with every operation in `dtype`; the margin is the smallest
    distance of any decision the pixel took from its threshold -- the snap tests on fx and fy (pixels), each in-frame tap's depth test (relative) and
    normal test, and t against 0 (relative to the distance)"""
    t = dtype
    tol, ncos, maxh, flags = t(np.float32(params[0])), t(np.float32(params[1])), params[2], params[3]
    H, W = cur[0].shape[:2]

    def split(accum, geom, albedo, ids):
        cfb, cf = accum[..., 3].view(np.int32), albedo[..., 3].view(np.int32)
        empty = (cfb == 0) | (cf == 0)
        nfb, nf = np.where(empty, 1, cfb).astype(t)[..., None], np.where(empty, 1, cf).astype(t)[..., None]
        C, M = accum[..., :3].astype(t) / nfb, albedo[..., :3].astype(t) / nf + t(EPS)
        return empty, ~np.isfinite(C).all(-1), (C / M if flags & DEMODULATE else C), geom[..., :3].astype(t) / nf, geom[..., 3].astype(t) / nf[..., 0], M, ids[..., 0] & 0x3FFFFFFF, cfb

    with np.errstate(all="ignore"):
        empty, bad, I, n, z, M, s, _ = split(*cur)
        he, hb, hI, hn, hz, _, hs, hcnt = split(*hist)
        c, p = cam_cur.astype(t), cam_prev.astype(t)
        yy, xx = np.mgrid[0:H, 0:W]
        aspect = t(W) / t(H)
        a, b = -(xx - W // 2).astype(t) / t(2 * W) * aspect, -(yy - H // 2).astype(t) / t(2 * H)
        v = (c[3:6] * a[..., None] + c[6:9] * b[..., None]) + c[9:12] * c[12]
        P = c[0:3] + v * (t(1) / np.sqrt(dot3(v, v)))[..., None] * z[..., None]
        d = P - p[0:3]
        tt, z_exp = dot3(d, p[9:12]), np.sqrt(dot3(d, d))
        live = ~empty & (tt > 0)
        margin = np.where(empty, np.inf, np.abs(tt) / z_exp)
        f, taps = [], live
        for k, (size, axis) in enumerate(((W, p[3:6]), (H, p[6:9]))):
            g = t(size // 2) - dot3(d, axis) * p[12] / tt * t(2 * size) / (aspect if k == 0 else t(1))
            r = np.rint(g)
            margin = np.minimum(margin, np.where(live, np.abs(np.abs(g - r) - SNAP), np.inf))
            g = np.where(np.abs(g - r) <= t(SNAP), r, g)
            taps = taps & (g >= -1) & (g < size)
            f.append(np.where(taps, g, 0))
        x0, y0 = np.floor(f[0]), np.floor(f[1])
        tx, ty = f[0] - x0, f[1] - y0
        sw, acc, Nh = np.zeros((H, W), t), np.zeros((H, W, 3), t), np.full((H, W), 1 << 30)
        miss = s == 0x3FFFFFFF
        for k in range(4):
            qx, qy = x0.astype(np.int64) + (k & 1), y0.astype(np.int64) + (k >> 1)
            w = (tx if k & 1 else t(1) - tx) * (ty if k >> 1 else t(1) - ty)
            use = taps & (w != 0) & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            q = (np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1))
            seen = use & ~he[q]
            valid = seen & ~hb[q] & (hs[q] == s)
            if tol > 0:
                dz = np.abs(hz[q] - z_exp)
                valid, margin = valid & (dz <= tol * z_exp), np.minimum(margin, np.where(seen, np.abs(dz - tol * z_exp) / z_exp, np.inf))
            if ncos > -1:
                dn = dot3(n, hn[q])
                valid, margin = valid & (miss | (dn >= ncos)), np.minimum(margin, np.where(seen & ~miss, np.abs(dn - ncos), np.inf))
            sw, acc, Nh = sw + np.where(valid, w, t(0)), acc + np.where(valid[..., None], w[..., None] * hI[q], t(0)), np.where(valid, np.minimum(Nh, hcnt[q]), Nh)
        has = sw > 0
        Ih = acc / np.where(has, sw, t(1))[..., None]
        N = np.where(empty, 0, np.where(has, np.where(bad, Nh, np.minimum(Nh + 1, maxh)), np.where(bad, 0, 1)))
        blend = Ih + (I - Ih) / np.maximum(N, 1).astype(t)[..., None]
        out = np.where((has & bad)[..., None], Ih, np.where(has[..., None], blend, I))
        out = np.where((N == 0)[..., None], t(0), out * M if flags & DEMODULATE else out)
        return out * N.astype(t)[..., None], N, margin


def error(got_sum, got_n, ref_sum, ref_n, compared):
    """max |got - ref64| / max(1, max |ref64|) over the compared pixels of non-zero count, on sum / N"""
    m = compared & (ref_n > 0)
    if not m.any():
        return 0.0
    ref = ref_sum[m] / ref_n[m][:, None]
    return float(np.abs(got_sum[m].astype(np.float64) / got_n[m][:, None] - ref).max() / max(1.0, np.abs(ref).max()))


def excluded(margin, cur):
    """(the compared pixels, the share of the non-empty pixels left out because a decision fell within MARGIN of its threshold)"""
    live = np.isfinite(margin) | (margin == np.inf) & ((cur[0][..., 3].view(np.int32) != 0) & (cur[2][..., 3].view(np.int32) != 0))
    compared = ~(margin < MARGIN)
    return compared, float((live & ~compared).sum()) / max(int(live.sum()), 1)
