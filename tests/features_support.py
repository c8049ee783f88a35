"""Shared by the feature-buffer tests (a NumPy model over the oracle; no test in here).

rtw_render_features (include/rtwin.h): per pixel the depth, shading normal, base colour and ids of what its camera rays meet first.  The model takes
the sample rays from camera_support.model_rays / lens_support.model_rays, the hit values from oracle.Scene.trace_closest (normal = hits[:, 3:6],
depth = hits[:, 6], shape, triangle) and the albedo from oracle.Scene.ray_trace(rays, keys, 1, True, ...); the values of a miss (depth 1000, normal 0,
triangle -1) it fills in itself from shape < 0.  Per pass a channel takes (v_0 + ... + v_{ns-1}) / ns, summed left to right in float32 from +0, no
division when ns == 1; the passes are added in order; the ids are those of sub-sample 0 of the last pass.  Only the pixels of the rank's tasks change.

As for camera_support: oracle.ray_trace restarts a path's counter at 0 where a frame's path stands at 2 after its camera ray, so the scenes the
model can follow hold no Blend (the only material node whose PREVIEW draws a random number)."""
import numpy as np

import camera_support as CS
import lens_support as LS
import scenes as SC

f32 = np.float32
SEED = 12345


def quirk_no_blend():
    """scenes.quirk_scene() -- a textured mesh first, analytic shapes in front of it that keep its texel -- with the one Blend (the plane's) replaced by
    its diffuse operand, so that the oracle's explicit-ray entry can follow the preview colour (module docstring).  Geometry and order unchanged."""
    out = []
    for sh in SC.quirk_scene():
        mat = sh[-1]
        if mat is not None and any(n[0] == SC.BL for n in mat):
            mat = SC.diffuse((1.0, 0.9, 0.8))
        out.append(sh[:-1] + (mat,))
    return out


def product_scene(R, O, ctx, shapes, asset):
    """camera_support.product_scene for every shape kind of tests/scenes.py (capsules and triangles too)"""
    s = R.RayTracerScene(ctx)
    for sh in shapes:
        mat = None if sh[-1] is None else R.material_nodes_from_array(O.materials(sh[-1]))
        make = {"sphere": lambda: R.RSphere.Create(sh[1], sh[2]), "plane": lambda: R.RPlane.Create(sh[1], sh[2]),
                "capsule": lambda: R.RCapsule.Create(sh[1], sh[2], sh[3]), "triangle": lambda: R.RTriangle.Create(sh[1], sh[2], sh[3]),
                "mesh": lambda: R.RMeshShape.Create(asset(sh[1] + ".obj"))}
        s.AddShape(make[sh[0]](), mat)
    return s


def share_pixels(W, H, task_rows, rank, world):
    """pixels of the rank's tasks (task t = rows t * task_rows .., owned by rank t % world), ascending"""
    rows = [y for y in range(H) if (y // task_rows) % world == rank]
    return (np.asarray(rows, np.int64)[:, None] * W + np.arange(W, dtype=np.int64)[None, :]).reshape(-1)


def sample_rays(cam, lens, W, H, pix, pass_index, sub, seed):
    if lens is not None and float(lens[0]) > 0.0:
        return LS.model_rays(cam, lens, W, H, pix, pass_index, sub, seed)
    return CS.model_rays(cam, W, H, pix, pass_index, sub, seed)


def cleared(W, H):
    """(geom, albedo, ids) as rtw_features_clear leaves them, in the layout FeatureBuffers.read() returns: the count as a float"""
    return np.zeros((W * H, 4), f32), np.zeros((W * H, 4), f32), np.full((W * H, 2), -1, np.int32)


_frames = {}


def model(O, asset, shapes, cam, lens, W, H, ns, first_pass=0, n_passes=1, seed=SEED, task_rows=10, rank=0, world=1, into=None):
    """(geom (W*H, 4), albedo (W*H, 4) with the count as a float, ids (W*H, 2)) after one call on top of `into` (default: cleared buffers).
    Results on cleared buffers are computed once per key and must not be written to."""
    key = (repr(shapes), np.asarray(cam, f32).tobytes(), None if lens is None else np.asarray(lens, f32).tobytes(), W, H, ns, first_pass, n_passes,
           seed, task_rows, rank, world)
    if into is None and key in _frames:
        return _frames[key]
    sc = CS.oracle_scene(O, shapes, asset)
    geom, albedo, ids = [a.copy() for a in (cleared(W, H) if into is None else into)]
    pix = share_pixels(W, H, task_rows, rank, world)
    n = len(pix)
    sums = np.concatenate([geom[pix, 0:3], geom[pix, 3:4], albedo[pix, 0:3]], axis=1).astype(f32)       # normal.xyz, depth, albedo.rgb
    for p in range(first_pass, first_pass + n_passes):
        csum = np.zeros((n, 7), f32)
        for i in range(ns):
            rays = sample_rays(cam, lens, W, H, pix, p, i, seed)
            hits, shape, tri = sc.trace_closest(rays)
            keys = np.stack([pix, np.full(n, p * 4 + i)], 1).astype(np.uint32)
            rgb = sc.ray_trace(rays, keys, 1, True, seed, W, H)
            miss = shape < 0
            v = np.zeros((n, 7), f32)
            v[:, 0:3] = np.where(miss[:, None], f32(0.0), hits[:, 3:6])
            v[:, 3] = np.where(miss, rays[:, 6], hits[:, 6])
            v[:, 4:7] = rgb
            csum = (csum + v).astype(f32)
            if i == 0 and p == first_pass + n_passes - 1:
                ids[pix, 0] = np.where(miss, -1, shape)
                ids[pix, 1] = np.where(miss, -1, tri)
        c = csum if ns == 1 else (csum / f32(ns)).astype(f32)
        sums = (sums + c).astype(f32)
    if n_passes > 0:
        geom[pix, 0:3] = sums[:, 0:3]; geom[pix, 3] = sums[:, 3]
        albedo[pix, 0:3] = sums[:, 4:7]
        albedo[pix, 3] += f32(n_passes)
    out = (geom, albedo, ids)
    if into is None:
        _frames[key] = out
    return out


def same(got, want):
    """every bit of the seven float channels, the count and the ids"""
    return all((CS.bits(g) == CS.bits(w)).all() for g, w in zip(got, want))


def first_difference(got, want):
    """for an assertion message: which buffer, how many words differ, the first pixel and its values"""
    for name, g, w in zip(("geom", "albedo", "ids"), got, want):
        bad = np.argwhere(CS.bits(g) != CS.bits(w))
        if len(bad):
            px = int(bad[0][0])
            return "%s: %d words differ; first pixel %d: got %r want %r" % (name, len(bad), px, g[px].tolist(), w[px].tolist())
    return "equal"
