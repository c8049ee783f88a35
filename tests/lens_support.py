"""Shared by the lens tests (a NumPy model and a frame helper; no test in here).

The thin-lens ray of include/rtwin.h in float32, every product and every sum rounded on its own, and behind it the oracle's
explicit-ray entry (oracle.Scene.ray_trace), exactly as tests/camera_support.py does for the pinhole: model rays with keys
(pixel, pass * 4 + sub), the sub-samples summed in order, divided by their number, accumulated pass after pass.  The lens point
comes from a stream of its own, so a path's counter stands at 2 after its camera ray with or without a lens; the scenes the oracle
can follow are therefore the same (camera_support.TORUS / MIXED: no counter-stream random whose value matters)."""
import numpy as np

from camera_support import bits, f32, oracle_scene, rand31  # noqa: F401  (bits: for the tests that import this module)

LENS_STREAM = 0x80000000
TRIES = 8


def pick_lens_point(lx, ly):
    """(lx, ly, try) per sample from the candidates lx, ly of shape (TRIES, n): the first try inside the unit disc (the test is
    lx * lx + ly * ly <= 1 in float32), try = TRIES and the centre when there is none."""
    lx, ly = np.asarray(lx, f32), np.asarray(ly, f32)
    inside = ((lx * lx).astype(f32) + (ly * ly).astype(f32)).astype(f32) <= f32(1.0)
    first = np.where(inside.any(axis=0), inside.argmax(axis=0), TRIES)
    col = np.arange(lx.shape[1])
    t = np.minimum(first, TRIES - 1)
    ok = first < TRIES
    return np.where(ok, lx[t, col], f32(0.0)).astype(f32), np.where(ok, ly[t, col], f32(0.0)).astype(f32), first


def lens_points(pixels, pass_index, sub, seed):
    """the lens point of every pixel's sample and the index of the try that gave it"""
    pix = np.asarray(pixels, np.int64)
    sample = (pass_index * 4 + sub) | LENS_STREAM

    def u(c):
        return rand31(seed, pix, sample, c).astype(np.int32).astype(f32) / f32(2147483648.0)
    lx = np.stack([(f32(2.0) * u(2 * t) - f32(1.0)).astype(f32) for t in range(TRIES)])
    ly = np.stack([(f32(2.0) * u(2 * t + 1) - f32(1.0)).astype(f32) for t in range(TRIES)])
    return pick_lens_point(lx, ly)


def view_vectors(cam, W, H, pixels, pass_index, sub, seed):
    """v of include/rtwin.h (before it is normalised), jitter included: three (n,) arrays"""
    cam = np.asarray(cam, f32)
    right, up, fwd, focal = cam[3:6], cam[6:9], cam[9:12], cam[12]
    pix = np.asarray(pixels, np.int64)
    x, y = pix % W, pix // W
    aspect = f32(W) / f32(H)
    dx = -(x - W // 2).astype(f32) / f32(W * 2) * aspect
    dy = -(y - H // 2).astype(f32) / f32(H * 2)
    ipr = f32(1.0) / f32(W * 4)
    orad = ipr * f32(0.5)
    sample = pass_index * 4 + sub
    u0 = rand31(seed, pix, sample, 0).astype(np.int32).astype(f32) / f32(2147483648.0)
    u1 = rand31(seed, pix, sample, 1).astype(np.int32).astype(f32) / f32(2147483648.0)
    ox = (ipr if sub & 1 else f32(0.0)) + (u0 - f32(0.5)) * orad
    oy = (ipr if sub & 2 else f32(0.0)) + (u1 - f32(0.5)) * orad
    a, b = (dx + ox).astype(f32), (dy + oy).astype(f32)
    return [((right[k] * a + up[k] * b) + fwd[k] * focal).astype(f32) for k in range(3)]


def model_rays(cam, lens, W, H, pixels, pass_index, sub, seed):
    """The lens ray of include/rtwin.h in float32: (n, 7) rays.  lens = (aperture_radius, focus_distance), radius > 0."""
    cam = np.asarray(cam, f32)
    eye, right, up, focal = cam[0:3], cam[3:6], cam[6:9], cam[12]
    radius, focus = f32(lens[0]), f32(lens[1])
    pix = np.asarray(pixels, np.int64)
    v = view_vectors(cam, W, H, pix, pass_index, sub, seed)
    lx, ly, _ = lens_points(pix, pass_index, sub, seed)
    s = focus / focal
    lxr, lyr = (lx * radius).astype(f32), (ly * radius).astype(f32)
    rays = np.zeros((len(pix), 7), f32)
    w = []
    for k in range(3):
        off = ((right[k] * lxr).astype(f32) + (up[k] * lyr).astype(f32)).astype(f32)
        rays[:, k] = (eye[k] + off).astype(f32)
        w.append(((v[k] * s).astype(f32) - off).astype(f32))
    sq = (((w[0] * w[0]).astype(f32) + (w[1] * w[1]).astype(f32)).astype(f32) + (w[2] * w[2]).astype(f32)).astype(f32)
    inv = (f32(1.0) / np.sqrt(sq)).astype(f32)
    for k in range(3):
        rays[:, 3 + k] = (w[k] * inv).astype(f32)
    rays[:, 6] = f32(1000.0)
    return rays


def target_distance(pose):
    """distance from a pose's eye to its target (camera_support.POSES entry): the focus distance the frame tests use"""
    eye, target = np.asarray(pose[0], np.float64), np.asarray(pose[1], np.float64)
    return float(np.sqrt(((target - eye) ** 2).sum()))


_frames = {}


def oracle_frame(O, asset, shapes, cam, lens, W, H, ns, depth, preview=False, first_pass=0, n_passes=1, seed=12345, begin=0, end=None):
    """camera_support.oracle_frame with the lens ray: (accumulator (W*H, 4), ARGB (W*H,)) of the passes over the pixels begin .. end,
    rendered into a cleared framebuffer.  Computed once per key."""
    end = W * H - 1 if end is None else end
    key = (repr(shapes), np.asarray(cam, f32).tobytes(), np.asarray(lens, f32).tobytes(), W, H, ns, depth, bool(preview), first_pass, n_passes, seed, begin, end)
    if key in _frames:
        return _frames[key]
    sc = oracle_scene(O, shapes, asset)
    pix = np.arange(begin, end + 1, dtype=np.int64)
    total = np.zeros((len(pix), 3), f32)
    c = np.zeros((len(pix), 3), f32)
    for p in range(first_pass, first_pass + n_passes):
        csum = np.zeros((len(pix), 3), f32)
        for i in range(ns):
            rays = model_rays(cam, lens, W, H, pix, p, i, seed)
            keys = np.stack([pix, np.full(len(pix), p * 4 + i)], 1).astype(np.uint32)
            csum = (csum + sc.ray_trace(rays, keys, depth, preview, seed, W, H)).astype(f32)
        c = csum if ns == 1 else (csum / f32(ns)).astype(f32)
        total = (total + c).astype(f32)
    accum = np.zeros((W * H, 4), f32)
    argb = np.zeros(W * H, np.uint32)
    if preview:
        argb[pix] = O.make_pixel_colors(c)
    else:
        accum[pix, :3] = total
        accum[pix, 3] = n_passes
        argb[pix] = O.make_pixel_colors(total if n_passes == 1 else (total / f32(n_passes)).astype(f32))
    _frames[key] = (accum, argb)
    return _frames[key]
