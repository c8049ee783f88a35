"""rtw_upsample on the GPU over wrapped torch tensors against the float64 NumPy evaluation of include/rtwin.h's formula (tests/upsample_support.py):
the value, the count, the exact gamma pack, untouched sources, and the direct and staged variants bit for bit.

Figures: the GPU's largest error over upsample_support.CASES is 3.443e-06 (74x46 from 37x23, sigmas 0.05 / 0.01) of the bound 2.685e-05."""
import numpy as np
import pytest

import upsample_support as US

pytestmark = pytest.mark.gpu
BOUND = 2.685e-05       # 8 x the largest float32-vs-float64 NumPy error over US.CASES (3.356e-06, 74x46 from 37x23 with sigmas 0.05 / 0.01)
IDS = dict(ids=lambda v: "x".join("%g" % x for x in v) if isinstance(v, tuple) else str(v))


@pytest.fixture(scope="module")
def ctx():
    import torch
    import raytracerwin_amd as R
    torch.cuda.init()
    c = R.Context(0, stream=torch.cuda.current_stream().cuda_stream)       # the wrapped tensors are written on torch's stream
    yield c
    c.close()


def run(ctx, lo, f_hi, params, stagings=(-1, 0, 1)):
    """[(accum (H, W, 4) with the count as a float, argb (H * W,)) per staging], the device copies of the seven inputs afterwards, and the objects"""
    import torch
    import raytracerwin_amd as R
    (h, w), (H, W) = lo[0].shape[:2], f_hi[0].shape[:2]
    dev = [torch.from_numpy(a).cuda() for a in lo + f_hi]
    out_a, argb = torch.full((H, W, 4), 7.0, device="cuda"), [torch.zeros((h, w), dtype=torch.int32, device="cuda"), torch.zeros((H, W), dtype=torch.int32, device="cuda")]
    fbs = [R.Framebuffer(ctx, w, h, dev[0].data_ptr(), argb[0].data_ptr()), R.Framebuffer(ctx, W, H, out_a.data_ptr(), argb[1].data_ptr())]
    feats = [R.FeatureBuffers.wrap(ctx, *dev[1:4]), R.FeatureBuffers.wrap(ctx, *dev[4:7])]
    got = []
    for s in stagings:
        ctx.set_option("upsample_staging", s)
        R.upsample(fbs[0], feats[0], feats[1], fbs[1], R.UpsampleParams(sigma_normal=params[0], sigma_depth=params[1], flags=params[2]))
        got.append((fbs[1].read_float().reshape(H, W, 4), fbs[1].resolve_argb()))
    ctx.set_option("upsample_staging", -1)
    return got, [d.cpu().numpy() for d in dev], (fbs, feats, out_a)


def check(ctx, lo, f_hi, params):
    from raytracerwin_amd import api
    got, after, _ = run(ctx, lo, f_hi, params)
    ref, count, rounds, margin = US.reference(lo, f_hi, params)
    keep, share = US.compared(rounds, margin)
    accum, argb = got[0]
    err = US.error(accum[..., :3], ref, keep)
    print("error %.3e of bound %.3e, excluded %.4f, rounds %s" % (err, BOUND, share, np.bincount(rounds.ravel(), minlength=4)))
    assert share <= US.CAP and err <= BOUND
    assert (accum[..., 3] == count)[keep].all() and (accum[..., :3][accum[..., 3] == 0] == 0).all()
    assert (argb == US.pack(api.gamma_thresholds(), accum[..., :3].reshape(-1, 3))).all()
    for a, b in zip(lo + f_hi, after):
        assert (a.view(np.uint32) == b.view(np.uint32)).all()
    for a, c in got[1:]:
        assert (a.view(np.uint32) == accum.view(np.uint32)).all() and (c == argb).all()
    return accum


@pytest.mark.parametrize("W,H,w,h,params", US.CASES, **IDS)
def test_upsample_equals_the_formula(ctx, W, H, w, h, params):
    check(ctx, *US.inputs(W, H, w, h), params)


@pytest.mark.parametrize("W,H,w,h", [(37, 23, 37, 23), (74, 46, 37, 23)])
def test_a_pixel_on_a_low_pixel_returns_its_mean_colour(ctx, W, H, w, h):
    """no sigmas, no flags: at ratio r the pixels with x = W/2 and y = H/2 modulo r read one tap of weight 1 (every pixel at equal sizes)"""
    lo, f_hi = US.inputs(W, H, w, h)
    accum, r = check(ctx, lo, f_hi, US.PLAIN), W // w
    ys, xs = np.mgrid[H // 2 % r:H:r, W // 2 % r:W:r]
    qy, qx = (ys - H // 2) // r + h // 2, (xs - W // 2) // r + w // 2
    C = lo[0][qy, qx, :3] / np.float32(2)
    on = (lo[0][qy, qx, 3].view(np.int32) > 0) & np.isfinite(C).all(-1) & (f_hi[1][ys, xs, 3].view(np.int32) > 0)
    assert on.sum() >= 700 and (accum[ys, xs, :3][on].view(np.uint32) == C[on].view(np.uint32)).all()


def test_upsample_of_rendered_frames(ctx):
    import raytracerwin_amd as R
    from conftest import asset
    s = R.RayTracerScene(ctx)
    s.AddShape(R.RMeshShape.Create(asset("TorusKnot.obj")), R.SurfaceMaterial_Diffuse((0.9, 0.6, 0.3)))
    frames = []
    for W, H in ((48, 27), (96, 54)):
        fb, feat = R.Framebuffer(ctx, W, H), R.FeatureBuffers(ctx, W, H)
        s.render_passes(fb, 10, 0, 1, 4, R.RenderOption(False), 0, 1, 1, 12345)
        s.render_features(feat, 10, 0, 1, 0, 1, 1, 12345)
        accum = fb.read_float().reshape(H, W, 4)
        accum[..., 3] = accum[..., 3].astype(np.int32).view(np.float32)          # back to the device's layout: the counts as int bits
        geom, albedo, ids = (a.reshape(H, W, -1) for a in feat.read())
        albedo[..., 3] = albedo[..., 3].astype(np.int32).view(np.float32)
        frames.append((accum, geom, albedo, ids))
    accum = check(ctx, frames[0], frames[1][1:], US.DEFAULTS)
    assert (accum[..., 3] == 1).all() and 0.0 < (frames[1][3][..., 0] >= 0).mean() < 1.0       # hits and misses, every pixel filled


def test_refusals_leave_the_destination_alone(ctx):
    import raytracerwin_amd as R
    _, _, ((lo, dst), (f_lo, f_hi), out_a) = run(ctx, *US.inputs(32, 16, 16, 8), US.DEFAULTS, stagings=())
    other, fb, ft = R.Context(0), lambda *a: R.Framebuffer(ctx, *a), lambda *a: R.FeatureBuffers(ctx, *a)
    bad = [(None, f_lo, f_hi, dst, {}), (lo, None, f_hi, dst, {}), (lo, f_lo, None, dst, {}), (lo, f_lo, f_hi, None, {}),
           (fb(48, 24), ft(48, 24), f_hi, dst, {}), (fb(3, 2), ft(3, 2), f_hi, dst, {}), (fb(16, 9), ft(16, 9), f_hi, dst, {}),      # w > W, W > 8 w, another aspect
           (fb(16384, 1), ft(16384, 1), ft(32768, 2), fb(32768, 2), {}),                                                           # W > 16384
           (lo, ft(16, 9), f_hi, dst, {}), (lo, f_lo, ft(32, 17), dst, {}), (R.Framebuffer(other, 16, 8), f_lo, f_hi, dst, {}), (lo, f_lo, R.FeatureBuffers(other, 32, 16), dst, {}),
           (dst, f_hi, f_hi, dst, {}), (fb(32, 16), f_hi, f_hi, dst, {}), (lo, f_lo, f_hi, dst, dict(sigma_normal=float("nan"))), (lo, f_lo, f_hi, dst, dict(sigma_depth=float("nan"))),
           (lo, f_lo, f_hi, dst, dict(flags=4))]
    for *args, kw in bad:
        with pytest.raises((R.RtwError, AttributeError)):
            R.upsample(*args, R.UpsampleParams(**kw))
    ctx.synchronize()
    assert (out_a.cpu().numpy() == 7.0).all()
    other.close()
