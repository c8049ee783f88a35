"""Shared by the tonemap tests (a NumPy model; no test in here).

rtw_tonemap / rtw_exposure_meter (include/rtwin.h): float32 with every product, sum and quotient rounded on its own, float64 where the formula says
double, integers elsewhere.  A state is (exposure float32, metered bool, frames int, hist (256,) uint32 of the last metered frame)."""
import numpy as np

from denoise_support import pack

f32 = np.float32
LINEAR, REINHARD, ACES, HOLD = 0, 1, 2, 1
FRESH = (f32(1.0), False, 0, np.zeros(256, np.uint32))
DEFAULTS = dict(curve=ACES, key=0.18, white=4.0, low_fraction=0.5, high_fraction=0.95, min_exposure=0.015625, max_exposure=64.0, adapt=0.25)


def lum(c):
    return ((f32(0.2126) * c[:, 0] + f32(0.7152) * c[:, 1]).astype(f32) + f32(0.0722) * c[:, 2]).astype(f32)


def synthetic(W, H, seed):
    """(W * H, 4) float32 accumulator, the count as int bits in w: luminances from 2^-24 to 2^14, every bin edge and the float below it, counts 0..5,
    and pixels whose luminance is 0, negative, NaN and +inf"""
    n, r = W * H, np.random.default_rng(seed)
    L = np.exp2(r.uniform(-24, 14, n)).astype(f32)
    edges = ((856 + np.arange(257, dtype=np.uint32)) << 20).astype(np.uint32)
    L[:514] = np.concatenate([edges, edges - np.uint32(1)]).view(f32)
    rgb = (L[:, None] * r.uniform(0.5, 1.5, (n, 3))).astype(f32)
    rgb[:514] = L[:514, None]                       # grey: lum rounds to within a bit of the edge, on either side
    rgb[514:522] = np.array([[0, 0, 0], [-1, -2, -3], [np.nan, 1, 1], [np.inf, 1, 1], [1, -np.inf, 2], [-0.5, 0.1, 0.2], [np.inf, np.inf, np.inf], [0, 0, 1e-30]], f32)
    cnt = r.integers(1, 6, n).astype(np.int32)
    cnt[r.choice(n, n // 16, replace=False)] = 0
    cnt[514:522] = 1
    with np.errstate(all="ignore"):
        acc = np.concatenate([(rgb * cnt[:, None].astype(f32)).astype(f32), cnt.view(f32)[:, None]], 1)
    return np.ascontiguousarray(acc, f32)


def frames():
    """tag -> (W, H, accumulator): 40 x 21 is one partial chunk of one block, 96 x 67 seven blocks with a ragged tail (two under "tonemap_blocks" 2)"""
    a, big = synthetic(40, 21, 1), synthetic(96, 67, 2)
    black = np.zeros((840, 4), f32)
    black[:, 3] = np.int32(1).view(f32)
    dim, lit = a.copy(), a.copy()
    dim[:, :3] *= f32(2.0 ** -7)
    lit[:, :3] *= f32(32.0)
    return {"syn40": (40, 21, a), "syn96": (96, 67, big), "dim40": (40, 21, dim), "lit40": (40, 21, lit), "black40": (40, 21, black)}


# A case is a run of steps through ONE exposure object, reset before the first.  A step: frame, mode, "tonemap_histogram", "tonemap_blocks", parameters.
# Modes: auto = tonemap with the object; null = without one; hold = set(2.5), then HOLD; meter = meter only; inplace = auto with dst = src.
# (fractions 0.9 and 0.9001 of 6 000 pixels truncate to one integer: the window falls back to the whole histogram)
HALF = dict(adapt=0.5)
CASES = {
    "one_block_linear": [("syn40", "auto", 0, 0, dict(curve=LINEAR))],
    "one_block_reinhard_aggregated": [("syn40", "auto", 1, 0, dict(curve=REINHARD, white=2.0))],
    "seven_blocks_aces_twice": [("syn96", "auto", 0, 0, {}), ("syn96", "auto", 0, 0, {})],
    "seven_blocks_aggregated": [("syn96", "auto", 1, 0, dict(curve=REINHARD, low_fraction=0.0, high_fraction=1.0))],
    "two_blocks_stride": [("syn96", "auto", 1, 2, {}), ("syn96", "auto", 0, 2, dict(curve=LINEAR, low_fraction=0.9, high_fraction=0.9001))],
    "no_exposure_object": [("syn40", "null", 0, 0, {})],
    "hold_after_set": [("syn40", "hold", 0, 0, dict(curve=REINHARD))],
    "meter_then_in_place": [("syn96", "meter", 1, 0, {}), ("syn96", "inplace", 0, 0, {})],
    "three_frames_then_black": [("syn40", "auto", 0, 0, HALF), ("dim40", "auto", 1, 0, HALF), ("lit40", "auto", 0, 0, HALF), ("black40", "auto", 1, 0, HALF)],
}
PATTERN = (f32(7.0), np.uint32(0x01020304))        # what a destination holds before a step: a pixel of count 0 must keep it


def expected(case, thr):
    """per step of the case: (state after, accum (n, 4) count as int bits, argb) by the model, from a fresh exposure object"""
    fr, state, out = frames(), FRESH, []
    for frame, mode, _, _, kw in CASES[case]:
        acc = fr[frame][2]
        into = (acc, np.full(len(acc), PATTERN[1])) if mode == "inplace" else (np.full(acc.shape, PATTERN[0]), np.full(len(acc), PATTERN[1]))
        if mode == "hold":
            state = (f32(2.5), True) + state[2:]
        after, img = model(acc, FRESH if mode == "null" else state, kw, thr, into, meter=mode in ("auto", "meter", "inplace"), write=mode != "meter")
        state = state if mode == "null" else after
        out.append((state, img[0], img[1]))
    return out


def same(state, accum, argb, want):
    """the bits of one step's results against expected()'s"""
    (E, _, n, hist), wa, wr = want
    return (np.float32(state[0]).view(np.uint32) == E.view(np.uint32) and state[1] == n and (state[2] == hist).all()
            and (accum.view(np.uint32) == wa.view(np.uint32)).all() and (argb == wr).all())


def histogram(acc):
    cnt = acc[:, 3].view(np.int32)
    with np.errstate(all="ignore"):
        L = lum((acc[:, :3] / cnt[:, None].astype(f32)).astype(f32))
    ok = (cnt != 0) & (L > 0) & np.isfinite(L)
    bins = np.clip((L.view(np.uint32) >> 20).astype(np.int64) - 856, 0, 255)
    return np.bincount(bins[ok], minlength=256).astype(np.uint32)


def new_state(state, h, p):
    E, metered, frames, last = state
    N = int(h.sum())
    if N == 0:
        return state
    lo, hi = int(np.float64(f32(p["low_fraction"])) * N), int(np.float64(f32(p["high_fraction"])) * N)
    if hi <= lo:
        lo, hi = 0, N
    P = np.concatenate([[0], np.cumsum(h.astype(np.int64))])
    c = np.maximum(np.minimum(P[1:], hi) - np.maximum(P[:-1], lo), 0)
    m = np.float64(int((np.arange(256) * c).sum())) / np.float64(hi - lo)
    t = np.uint32(int(((m + 0.5) + 856.0) * 1048576.0))
    target = np.fmin(np.fmax(f32(p["key"]) / t.view(f32), f32(p["min_exposure"])), f32(p["max_exposure"]))
    E = f32(E + f32(f32(target - E) * f32(p["adapt"]))) if metered else f32(target)
    return (E, True, frames + 1, h.copy())


def mapped(acc, E0, p, thr, into):
    """(accum (n, 4) with the count as int bits, argb (n,)): `into` with every pixel of non-zero count replaced"""
    cnt = acc[:, 3].view(np.int32)
    with np.errstate(all="ignore"):
        x = ((acc[:, :3] / cnt[:, None].astype(f32)).astype(f32) * f32(E0)).astype(f32)
        if p["curve"] == REINHARD:
            lx, ww = lum(x), f32(f32(p["white"]) * f32(p["white"]))
            s = np.where(lx > 0, ((f32(1) + (lx / ww).astype(f32)).astype(f32) / (f32(1) + lx).astype(f32)).astype(f32), f32(1))
            x = (x * s[:, None]).astype(f32)
        elif p["curve"] == ACES:
            v = np.fmax(x, f32(0))
            num = (v * ((f32(2.51) * v).astype(f32) + f32(0.03)).astype(f32)).astype(f32)
            den = ((v * ((f32(2.43) * v).astype(f32) + f32(0.59)).astype(f32)).astype(f32) + f32(0.14)).astype(f32)
            x = (num / den).astype(f32)
    live = cnt != 0
    accum, argb = into[0].copy(), into[1].copy()
    accum[live, :3] = x[live]
    accum[live, 3] = np.int32(1).view(f32)
    argb[live] = pack(thr, x[live])
    return accum, argb


def model(acc, state, p, thr, into, meter=True, write=True):
    """one call: (state after, (accum, argb) of dst after, or `into` for a meter-only call)"""
    p = dict(DEFAULTS, **p)
    out = mapped(acc, state[0], p, thr, into) if write else into
    return (new_state(state, histogram(acc), p) if meter else state), out
