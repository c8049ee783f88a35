"""rtw_reproject on the GPU over wrapped torch tensors against the float64 NumPy evaluation of include/rtwin.h's formula (tests/reproject_support.py):
the value, the history length, the exact gamma pack, untouched sources, and the direct and staged variants bit for bit."""
import numpy as np
import pytest

import reproject_support as RS

pytestmark = pytest.mark.gpu
# 8 x the largest error of the float32 NumPy evaluation against the float64 one over all these cases (1.305e-05, 131x70 roll: profiles/reproject_experiments.md section 1)
BOUND = 1.044e-04
CAP = 0.03              # at most this share of the non-empty pixels may decide within RS.MARGIN of a threshold and be left out of the comparison


@pytest.fixture(scope="module")
def ctx():
    import torch
    import raytracerwin_amd as R
    torch.cuda.init()
    c = R.Context(0, stream=torch.cuda.current_stream().cuda_stream)       # the wrapped tensors are written on torch's stream
    yield c
    c.close()


def camera(a):
    import raytracerwin_amd as R
    return R.Camera.from_buffer_copy(np.ascontiguousarray(a, np.float32).tobytes())


def run(ctx, cams, cur, hist, params, stagings=(-1, 0, 1)):
    """[(accum (H, W, 4) with the count as a float, argb (H * W,)) per variant], the device copies of the eight inputs afterwards, and the objects"""
    import torch
    import raytracerwin_amd as R
    H, W = cur[0].shape[:2]
    dev = [torch.from_numpy(a).cuda() for a in cur + hist]
    out_a, argb = torch.full((H, W, 4), 7.0, device="cuda"), [torch.full((H, W), 7, dtype=torch.int32, device="cuda") for _ in range(3)]
    fbs = [R.Framebuffer(ctx, W, H, a.data_ptr(), c.data_ptr()) for a, c in zip((dev[0], dev[4], out_a), argb)]
    feats = [R.FeatureBuffers.wrap(ctx, *dev[1:4]), R.FeatureBuffers.wrap(ctx, *dev[5:8])]
    p = R.ReprojectParams(depth_tolerance=params[0], normal_cos=params[1], max_history=params[2], flags=params[3])
    got = []
    for s in stagings:
        ctx.set_option("reproject_staging", s)
        R.reproject(camera(cams[0]), camera(cams[1]), fbs[0], feats[0], fbs[1], feats[1], fbs[2], p)
        got.append((fbs[2].read_float().reshape(H, W, 4), fbs[2].resolve_argb()))
    ctx.set_option("reproject_staging", -1)
    return got, [d.cpu().numpy() for d in dev], (fbs, feats, out_a)


def check(ctx, cams, cur, hist, params):
    """-> (N, the reference's N)"""
    from raytracerwin_amd import api
    got, after, _ = run(ctx, cams, cur, hist, params)
    ref_sum, ref_n, margin = RS.reference(cams[0], cams[1], cur, hist, params)
    compared, share = RS.excluded(margin, cur)
    accum, argb = got[0]
    n = accum[..., 3].astype(np.int64)
    err = RS.error(accum[..., :3], n, ref_sum, ref_n, compared)
    print("error %.3e of bound %.3e, excluded %.4f, N differs on %d compared pixels" % (err, BOUND, share, (n != ref_n)[compared].sum()))
    assert share <= CAP and err <= BOUND
    assert (n == ref_n)[compared].all()
    with np.errstate(all="ignore"):
        assert (argb == RS.pack(api.gamma_thresholds(), (accum[..., :3] / accum[..., 3:]).reshape(-1, 3))).all()
    for a, b in zip(cur + hist, after):
        assert (a.view(np.uint32) == b.view(np.uint32)).all()
    for a, c in got[1:]:
        assert (a.view(np.uint32) == accum.view(np.uint32)).all() and (c == argb).all()
    return accum, ref_n


@pytest.mark.parametrize("W,H,pair,params", RS.CASES, ids=lambda v: "-".join("%g" % x for x in v) if isinstance(v, tuple) else str(v))
def test_reproject_equals_the_formula(ctx, W, H, pair, params):
    cc, cp, cleared = RS.PAIRS[pair]
    check(ctx, (cc, cp), *RS.inputs(W, H, cc, cp, cleared), params)


@pytest.mark.parametrize("W,H", RS.FRAMES)
def test_an_unmoved_camera_reads_one_tap_exactly(ctx, W, H):
    cur, hist = RS.inputs(W, H, RS.HOME, RS.HOME)
    accum, _ = check(ctx, (RS.HOME, RS.HOME), cur, hist, RS.EXACT)
    f32, nh = np.float32, hist[0][..., 3].view(np.int32)
    both = (nh > 0) & np.isfinite(cur[0][..., :3]).all(-1)
    n = np.minimum(nh + 1, RS.EXACT[2])[both]
    assert both.any() and (accum[..., 3][both] == n).all()
    C, Ih = cur[0][..., :3][both] / f32(2), hist[0][..., :3][both] / nh[both].astype(f32)[:, None]
    want = (Ih + (C - Ih) / n.astype(f32)[:, None]) * n.astype(f32)[:, None] / n.astype(f32)[:, None]
    assert ((accum[..., :3][both] / accum[..., 3:][both]).view(np.uint32) == want.astype(f32).view(np.uint32)).all()


def test_reproject_of_rendered_frames(ctx):
    import raytracerwin_amd as R
    from conftest import asset
    W, H = 96, 54
    s = R.RayTracerScene(ctx)
    s.AddShape(R.RMeshShape.Create(asset("TorusKnot.obj")), R.SurfaceMaterial_Diffuse((0.9, 0.6, 0.3)))
    cams = [R.Camera.look_at((0.4, 0.3, 7.0), (0.0, 0.0, 0.0)), R.Camera.look_at((0.0, 0.0, 7.0), (0.0, 0.0, 0.0))]       # current, previous: 4 degrees apart
    frames = []
    for k, cam in enumerate(cams):
        fb, feat = R.Framebuffer(ctx, W, H), R.FeatureBuffers(ctx, W, H)
        s.set_camera(cam)
        s.render_passes(fb, 10, 0, 1, 4, R.RenderOption(False), k, 1, 1, 12345)
        s.render_features(feat, 10, 0, 1, k, 1, 1, 12345)
        accum = fb.read_float().reshape(H, W, 4)
        accum[..., 3] = accum[..., 3].astype(np.int32).view(np.float32)          # back to the device's layout: the counts as int bits
        geom, albedo, ids = (a.reshape(H, W, -1) for a in feat.read())
        albedo[..., 3] = albedo[..., 3].astype(np.int32).view(np.float32)
        frames.append(((accum, geom, albedo, ids), fb, feat))
    accum, ref_n = check(ctx, [c.as_array() for c in cams], frames[0][0], frames[1][0], RS.DEFAULTS)
    assert 0.0 < (ref_n > 1).mean() < 1.0
    # three calls with an unmoved camera, from a cleared history: N = 1, 2, 3 (the current frame's features serve as the history's, in an object of their own)
    fb, feat, feat2 = frames[0][1], frames[0][2], R.FeatureBuffers(ctx, W, H)
    s.set_camera(cams[0])
    s.render_features(feat2, 10, 0, 1, 0, 1, 1, 12345)
    ping = [R.Framebuffer(ctx, W, H), R.Framebuffer(ctx, W, H)]
    ping[0].clear()
    for k in range(3):
        R.reproject(cams[0], cams[0], fb, feat, ping[k & 1], feat2, ping[(k + 1) & 1])
    n = ping[1].read_float().reshape(H, W, 4)[..., 3]
    inside = frames[0][0][3][..., 0] >= 0
    assert inside.any() and (n[inside] == 3).all()


def test_refusals_leave_the_destination_alone(ctx):
    import raytracerwin_amd as R
    cur, hist = RS.inputs(16, 8, RS.HOME, RS.HOME)
    _, _, ((fc, fh, dst), (tc, th), out_a) = run(ctx, (RS.HOME, RS.HOME), cur, hist, RS.DEFAULTS, stagings=())
    other, cam, flat = R.Context(0), camera(RS.HOME), camera(RS.HOME * np.float32(0.5))
    bad = [(cam, cam, None, tc, fh, th, dst, {}), (cam, cam, fc, tc, fh, th, None, {}), (cam, cam, dst, tc, fh, th, dst, {}), (cam, cam, fc, tc, dst, th, dst, {}),
           (cam, cam, fc, tc, fh, tc, dst, {}), (cam, cam, fc, tc, R.Framebuffer(ctx, 17, 8), th, dst, {}), (cam, cam, fc, R.FeatureBuffers(ctx, 16, 9), fh, th, dst, {}),
           (cam, cam, fc, tc, R.Framebuffer(other, 16, 8), th, dst, {}), (flat, cam, fc, tc, fh, th, dst, {}), (cam, flat, fc, tc, fh, th, dst, {}),
           (cam, cam, fc, tc, fh, th, dst, dict(depth_tolerance=float("nan"))), (cam, cam, fc, tc, fh, th, dst, dict(normal_cos=float("nan"))),
           (cam, cam, fc, tc, fh, th, dst, dict(max_history=0)), (cam, cam, fc, tc, fh, th, dst, dict(max_history=65536)), (cam, cam, fc, tc, fh, th, dst, dict(flags=2))]
    for *args, kw in bad:
        with pytest.raises((R.RtwError, AttributeError)):
            R.reproject(*args, R.ReprojectParams(**kw))
    ctx.synchronize()
    assert (out_a.cpu().numpy() == 7.0).all()
    other.close()
