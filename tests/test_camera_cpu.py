"""The camera's host side, runnable without a GPU: rtw_camera_rays against the NumPy model of the ray, look_at, the validation
rules, and the screen bins of general poses (the superset property of tests/test_host_cpu.py, generalised to eye and basis)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN, asset

import raytracerwin_amd as R
import camera_support as CS

f32 = np.float32
CPU_POSES = ["default", "offaxis", "below", "wide"]


def test_numpy_random_stream_is_the_oracles(oracle_mod):
    """a check of the test support only (it runs no product code and says nothing about the feature): the vectorised rand31 of
    tests/camera_support.py, which the ray model draws its jitter from, is oracle.rand31"""
    rng = np.random.default_rng(3)
    for _ in range(300):
        seed, pixel, sample, counter = (int(v) for v in rng.integers(0, 2 ** 32, 4))
        assert int(CS.rand31(seed, [pixel], sample, counter)[0]) == oracle_mod.rand31(seed, pixel, sample, counter)


def test_model_with_the_default_pose_reproduces_the_oracles_own_frames(oracle_mod):
    """the test design itself: model rays + ray_trace + make_pixel_colors = render_range, accumulator and ARGB, full paths and preview"""
    O = oracle_mod
    W, H = 48, 27
    for shapes in (CS.TORUS, CS.MIXED):
        for preview, npass in ((False, 2), (True, 1)):
            fb = O.Framebuffer(W, H)
            sc = CS.oracle_scene(O, shapes, asset)
            for p in range(npass):
                sc.render_range(fb, 0, W * H - 1, 3, preview, p, 4, 777)
            oa, ob = fb.read()
            a, b = CS.oracle_frame(O, asset, shapes, CS.cam13(R, "default"), W, H, 4, 3, preview, 0, npass, 777)
            assert (CS.bits(a) == CS.bits(oa)).all() and (b == ob).all()


@pytest.mark.parametrize("pose", CPU_POSES)
@pytest.mark.parametrize("W,H", [(96, 54), (64, 200)])
def test_camera_rays_match_the_model_exactly(pose, W, H):
    cam = CS.camera_of(R, pose)
    pix = np.arange(W * H)
    for p in (0, 3):
        for sub in range(4):
            got = R.camera_rays(cam, W, H, pix, p, sub, 4242)
            want = CS.model_rays(cam.as_array(), W, H, pix, p, sub, 4242)
            assert (CS.bits(got) == CS.bits(want)).all(), (p, sub)


def test_look_at_the_reference_pose_is_the_default_struct():
    cam = R.Camera.look_at((0, 0, 7), (0, 0, 6), (0, 1, 0), 2.0 * math.degrees(math.atan(0.5)))
    want = np.array([0, 0, 7, 1, 0, 0, 0, 1, 0, 0, 0, -1, 0.5], f32)
    assert (CS.bits(cam.as_array()) == CS.bits(want)).all()
    assert cam == R.Camera.default()
    s = R.RayTracerScene(None)
    assert s.get_camera() == R.Camera.default()
    c = CS.camera_of(R, "below")
    s.set_camera(c)
    assert s.get_camera() == c
    s.set_camera(None)
    assert s.get_camera() == R.Camera.default()
    # look_at follows its definition: forward = normalized(target - eye), right = normalized(forward x up), up = right x forward
    eye, target, up, vfov = CS.POSES["below"]
    a = c.as_array().astype(np.float64)
    fw = np.subtract(target, eye) / np.linalg.norm(np.subtract(target, eye))
    rt = np.cross(fw, up) / np.linalg.norm(np.cross(fw, up))
    assert np.abs(a[9:12] - fw).max() < 1e-6 and np.abs(a[3:6] - rt).max() < 1e-6 and np.abs(a[6:9] - np.cross(rt, fw)).max() < 1e-6
    assert abs(a[12] - 0.25 / math.tan(math.radians(vfov) / 2)) < 1e-6 and (a[:3] == np.array(eye)).all()


def test_every_validation_rule_returns_its_error():
    def bad(fn, *args, **kw):
        with pytest.raises(R.RtwError) as e:
            fn(*args, **kw)
        assert e.value.code == -1
    nan, inf = float("nan"), float("inf")
    bad(R.Camera.look_at, (nan, 0, 7), (0, 0, 0))
    bad(R.Camera.look_at, (0, 0, 7), (0, inf, 0))
    bad(R.Camera.look_at, (0, 0, 7), (0, 0, 0), (0, nan, 0))
    bad(R.Camera.look_at, (0, 0, 7), (0, 0, 0), (0, 1, 0), nan)
    for vfov in (0.0, -10.0, 180.0, 200.0):
        bad(R.Camera.look_at, (0, 0, 7), (0, 0, 0), (0, 1, 0), vfov)
    bad(R.Camera.look_at, (1, 2, 3), (1, 2, 3))                      # target - eye is zero
    bad(R.Camera.look_at, (0, 0, 7), (0, 0, 0), (0, 0, -2.0))        # up hint parallel to forward
    bad(R.Camera.look_at, (0, 0, 7), (0, 0, 0), (0, 0, 0))
    s = R.RayTracerScene(None)
    good = CS.camera_of(R, "offaxis")

    def changed(field, k, v):
        c = R.Camera.from_buffer_copy(bytes(good))
        if field == "focal":
            c.focal = v
        else:
            getattr(c, field)[k] = v
        return c
    for c in (changed("eye", 1, nan), changed("right", 0, inf), changed("focal", 0, nan), changed("focal", 0, 0.0), changed("focal", 0, -0.5),
              changed("up", 1, good.up[1] + 3e-4),                    # not unit length
              changed("forward", 0, good.forward[0] * 1.001)):
        bad(s.set_camera, c)
        bad(R.camera_rays, c, 8, 8, [0])
    skew = R.Camera.from_buffer_copy(bytes(R.Camera.default()))
    skew.up[0], skew.up[1] = math.sin(3e-4), math.cos(3e-4)           # unit length, but 3e-4 off the right angle to `right`
    bad(s.set_camera, skew)
    ok = R.Camera.from_buffer_copy(bytes(R.Camera.default()))
    ok.up[0], ok.up[1] = math.sin(5e-5), math.cos(5e-5)               # inside the 1e-4 tolerance
    s.set_camera(ok)
    assert s.get_camera() == ok
    bad(R.camera_rays, good, 8, 8, [64])                              # pixel outside the frame
    bad(R.camera_rays, good, 8, 8, [0], 0, 4)


def _host_scene(name):
    s = R.RayTracerScene(None)
    s.AddShape(R.RMeshShape.Create(asset(name + ".obj")))
    return s


def test_default_camera_set_explicitly_gives_the_bins_of_no_camera():
    for name in ("TorusKnot", "BlenderMonkey"):
        a, b = _host_scene(name), _host_scene(name)
        b.set_camera(R.Camera.default())
        for W, H in ((192, 108), (64, 200)):
            (o0, e0), (o1, e1) = a.mesh_bins(W, H, 16, 4), b.mesh_bins(W, H, 16, 4)
            assert (o0 == o1).all() and (e0 == e1).all() and len(e0) > 0


def test_eye_inside_the_meshs_bounds_gets_no_bins():
    s = _host_scene("TorusKnot")
    s.set_camera(CS.camera_of(R, "inside"))
    assert s.mesh_bins(192, 108, 16, 4) is None
    s.set_camera(None)
    assert s.mesh_bins(192, 108, 16, 4) is not None      # ... of the scene's CURRENT camera


@pytest.mark.parametrize("name", ["TorusKnot", "BlenderMonkey"])
@pytest.mark.parametrize("pose", ["offaxis", "below"])
@pytest.mark.parametrize("W,H,step", [(192, 108, 3), (64, 200, 2)])
def test_screen_bins_of_a_general_pose_hold_every_triangle_a_camera_ray_can_accept(name, pose, W, H, step):
    """test_screen_bins_hold_every_triangle_a_camera_ray_can_accept of tests/test_host_cpu.py with the float64 Moeller-Trumbore test
    generalised to eye and basis: for camera rays of every sampled pixel -- jitter corners, centre and random offsets inside the
    sub-sample range -- every front-facing triangle the ray passes through must be in the pixel's bin."""
    bw, bh = 16, 4
    g = np.load(os.path.join(GOLDEN, "mesh_%s.npz" % name))
    s = _host_scene(name)
    cam = CS.camera_of(R, pose)
    s.set_camera(cam)
    bins_ = s.mesh_bins(W, H, bw, bh)
    assert bins_ is not None
    off, ent = bins_
    bounds, _, tri = s.mesh_nodes()
    assert len(off) == (W // bw) * (H // bh) + 1
    for b in range(len(off) - 1):
        e = ent[off[b]:off[b + 1]]
        assert (np.diff(e.astype(np.int64)) > 0).all() and (tri[e] >= 0).all()
    c13 = cam.as_array()
    eye, right, up, fwd, focal = c13[0:3], c13[3:6], c13[6:9], c13[9:12], c13[12]
    leaf_nodes = np.nonzero(tri >= 0)[0]
    P = g["points"].reshape(-1, 3).astype(np.float64)
    idx = g["pidx"].reshape(-1, 3)[tri[leaf_nodes]]
    p0, p1, p2 = P[idx[:, 0]], P[idx[:, 1]], P[idx[:, 2]]
    nrm = np.cross(p1 - p0, p2 - p0)
    o = eye.astype(np.float64)
    facing = ((o - p0) * nrm).sum(1) > 1e-7 * np.maximum(1e-30, np.linalg.norm(nrm, axis=1))     # clearly in front of the plane
    nn = np.int64(len(bounds))
    keys = np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(off.astype(np.int64))) * nn + ent.astype(np.int64)     # (bin, leaf) pairs
    rng = np.random.default_rng(7)
    r = f32(1.0) / f32(W * 4)
    pix = np.arange(0, W * H, step)
    xs, ys = pix % W, pix // W
    bins = ((ys // bh) * (W // bw) + xs // bw).astype(np.int64)
    offsets = [(-0.25, -0.25), (1.25, -0.25), (-0.25, 1.25), (1.25, 1.25), (0.5, 0.5)] + [tuple(rng.uniform(-0.25, 1.25, 2)) for _ in range(3)]
    e1, e2 = p1 - p0, p2 - p0
    aspect = f32(W) / f32(H)
    dx = -(xs - W // 2).astype(f32) / f32(W * 2) * aspect
    dy = -(ys - H // 2).astype(f32) / f32(H * 2)
    missing, seen = 0, 0
    for fx, fy in offsets:
        a, b = dx + f32(fx * r), dy + f32(fy * r)
        # the ray of include/rtwin.h in float32, before normalisation (which cannot change the line)
        d = np.stack([(right[k] * a + up[k] * b) + fwd[k] * focal for k in range(3)], 1).astype(np.float64)
        for c0 in range(0, len(xs), 1024):
            dd = d[c0:c0 + 1024]
            pv = np.cross(dd[:, None, :], e2[None])
            det = (e1[None] * pv).sum(2)
            ok = np.abs(det) > 1e-14
            inv = np.where(ok, 1.0 / np.where(ok, det, 1.0), 0.0)
            tv = (o - p0)[None]
            u = (tv * pv).sum(2) * inv
            qv = np.cross(tv, e1[None])
            v = (dd[:, None, :] * qv).sum(2) * inv
            t = (e2[None] * qv).sum(2) * inv
            hit = ok & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0) & facing[None]
            pi, li = np.nonzero(hit)
            seen += len(pi)
            missing += int((~np.isin(bins[c0 + pi] * nn + leaf_nodes[li], keys)).sum())
    assert seen > 0 and missing == 0, (seen, missing)
