"""Shared by the camera tests (data and a NumPy model; no test in here).

The oracle has no camera.  Its explicit-ray entry, oracle.Scene.ray_trace(rays, keys, ...), fed with a float32 model of the camera
ray (include/rtwin.h), stands in for one: model rays with keys (pixel, pass * 4 + sub), the sub-samples summed in order, divided
by their number, accumulated pass after pass, and oracle.make_pixel_colors for the ARGB words.  For the default pose this
reproduces oracle.render_range bit for bit (tests/test_camera_cpu.py checks it) as long as the scene draws no counter-stream
random whose value matters: no texture, no Blend, no Reflective with fuzziness > 0 -- ray_trace restarts a path's counter at 0
where a frame continues at 2.  The scenes below are of that class."""
import math

import numpy as np

import scenes as SC

f32 = np.float32
VFOV_DEFAULT = math.degrees(2.0 * math.atan(0.5))

# scenes (tests/scenes.py form) the oracle can follow with a moved camera
TORUS = [("mesh", "TorusKnot", SC.diffuse((1, 1, 1)))]                                   # the one-mesh path
MIXED = [("plane", (0.0, 1.0, 0.0), (0.0, -1.2, 0.0), SC.checker((0.9, 0.9, 0.9), 2.0)),    # the lead-shape path
         ("sphere", (1.9, 0.2, -0.5), 0.8, SC.reflective((0.9, 0.9, 0.9))),
         ("sphere", (-1.9, -0.3, 0.6), 0.6, SC.combine(SC.diffuse((0.2, 0.8, 0.3)), SC.emissive((0.3, 0.1, 0.1)))),
         ("mesh", "BlenderMonkey", SC.diffuse((0.9, 0.8, 0.7)))]
SCENES = {"torus": TORUS, "mixed": MIXED}
# textured mesh + Blend + a fuzzy mirror: outside that class, checked by agreement between the pipelines
FUZZY = [("sphere", (1.6, 0.4, 0.8), 0.7, SC.reflective((0.9, 0.9, 0.9), 0.2)),
         ("mesh", "unitychan", SC.blend(SC.reflective((1, 1, 1), 0.1), SC.diffuse((1.0, 1.0, 1.0)), 0.6))]

# poses: (eye, target, up hint, vfov in degrees); both meshes lie inside the box |x| < 1.4, |y| < 1, |z| < 1.1
POSES = {
    "offaxis": ((4.0, 2.5, 5.0), (0.1, -0.1, 0.0), (0.0, 1.0, 0.0), 40.0),         # the mesh wholly in front: bins
    "below": ((-2.5, -4.0, 3.0), (0.0, 0.2, 0.0), (0.35, 1.0, 0.2), 50.0),        # rolled, looking up from below
    "inside": ((0.2, 0.1, 0.3), (1.0, 0.3, -0.2), (0.0, 1.0, 0.0), 70.0),           # the eye inside the mesh's bounds: no bins
    "away": ((0.0, 0.0, 6.0), (8.66, 0.5, 1.0), (0.0, 1.0, 0.0), 30.0),             # turned 60 degrees away: the meshes in front of the eye plane but off screen (bins, all empty)
    "narrow": ((3.0, 1.0, 6.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 15.0),
    "wide": ((1.5, 1.2, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 100.0),
}


def camera_of(R, pose):
    """the library's camera struct of a pose name (None: no camera set, "default": the default set explicitly)"""
    if pose is None:
        return None
    if pose == "default":
        return R.Camera.default()
    eye, target, up, vfov = POSES[pose]
    return R.Camera.look_at(eye, target, up, vfov)


def cam13(R, pose):
    c = camera_of(R, pose)
    return (R.Camera.default() if c is None else c).as_array()


def product_scene(R, O, ctx, shapes, asset):
    s = R.RayTracerScene(ctx)
    for sh in shapes:
        mat = None if sh[-1] is None else R.material_nodes_from_array(O.materials(sh[-1]))
        if sh[0] == "sphere":
            s.AddShape(R.RSphere.Create(sh[1], sh[2]), mat)
        elif sh[0] == "plane":
            s.AddShape(R.RPlane.Create(sh[1], sh[2]), mat)
        else:
            s.AddShape(R.RMeshShape.Create(asset(sh[1] + ".obj")), mat)
    return s


# ---- the random stream (specification shared by the oracle and the library), vectorised ----
def _mix32(x):
    x = x.astype(np.uint32)
    x = x ^ (x >> np.uint32(16)); x = x * np.uint32(0x7feb352d)
    x = x ^ (x >> np.uint32(15)); x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def rand31(seed, pixel, sample, counter):
    """oracle.rand31 for arrays of pixels (tests/test_camera_cpu.py compares the two)"""
    with np.errstate(over="ignore"):
        h = _mix32(np.array([seed], np.uint32) ^ np.uint32(0x9E3779B9))
        h = _mix32(h + np.asarray(pixel).astype(np.uint32))
        key = _mix32(h + np.uint32(sample))
        return _mix32(key + np.uint32(counter)) >> np.uint32(1)


def model_rays(cam, W, H, pixels, pass_index, sub, seed):
    """The camera ray of include/rtwin.h in float32, every product and every sum rounded on its own: (n, 7) rays."""
    cam = np.asarray(cam, f32)
    eye, right, up, fwd, focal = cam[0:3], cam[3:6], cam[6:9], cam[9:12], cam[12]
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
    v = [((right[k] * a + up[k] * b) + fwd[k] * focal).astype(f32) for k in range(3)]
    sq = ((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]).astype(f32)
    inv = (f32(1.0) / np.sqrt(sq)).astype(f32)
    rays = np.zeros((len(pix), 7), f32)
    rays[:, 0:3] = eye
    for k in range(3):
        rays[:, 3 + k] = v[k] * inv
    rays[:, 6] = f32(1000.0)
    return rays


_oracle_scenes = {}


def oracle_scene(O, shapes, asset):
    key = repr(shapes)
    if key not in _oracle_scenes:
        _oracle_scenes[key] = O.Scene().add_shapes(shapes, lambda n: asset(n + ".obj"))
    return _oracle_scenes[key]


_frames = {}


def oracle_frame(O, asset, shapes, cam, W, H, ns, depth, preview=False, first_pass=0, n_passes=1, seed=12345, begin=0, end=None):
    """(accumulator (W*H, 4) as Framebuffer.read_float gives it, ARGB (W*H,)) of the passes first_pass .. first_pass + n_passes - 1 over
    the pixels begin .. end, rendered into a cleared framebuffer: the oracle's ray_trace behind the ray model.  Computed once per key."""
    end = W * H - 1 if end is None else end
    key = (repr(shapes), np.asarray(cam, f32).tobytes(), W, H, ns, depth, bool(preview), first_pass, n_passes, seed, begin, end)
    if key in _frames:
        return _frames[key]
    sc = oracle_scene(O, shapes, asset)
    pix = np.arange(begin, end + 1, dtype=np.int64)
    total = np.zeros((len(pix), 3), f32)
    c = np.zeros((len(pix), 3), f32)
    for p in range(first_pass, first_pass + n_passes):
        csum = np.zeros((len(pix), 3), f32)
        for i in range(ns):
            rays = model_rays(cam, W, H, pix, p, i, seed)
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


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)
