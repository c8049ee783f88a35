"""rtw_denoise_variance and rtw_reproject_moments on the GPU over wrapped torch tensors against the float64 NumPy evaluation of include/rtwin.h's
formulas (tests/variance_support.py): values, count, exact gamma pack, untouched sources, every tiling / prefilter route / staging bit for bit,
rtw_denoise's bits with sigma_lum = 0, rtw_reproject's bits in dst, and the refusals."""
import numpy as np
import pytest

import reproject_support as RS
import variance_support as VS
from variance_support import BOUND, BOUND_MOMENTS      # 8 x the float32 NumPy evaluation's own error: profiles/variance_experiments.md section 1

pytestmark = pytest.mark.gpu


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


def wrapped(ctx, arrays, mu):
    """(Framebuffer, FeatureBuffers, Moments, the tensors) over device copies of a frame's four arrays and its moments; None: all filled with 7"""
    import torch
    import raytracerwin_amd as R
    H, W = mu.shape[:2]
    dev = [torch.from_numpy(a).cuda() for a in tuple(arrays) + (mu,)] if arrays else [torch.full((H, W, 4), 7.0, device="cuda"), None, None, None, torch.full((H, W, 2), 7.0, device="cuda")]
    dev.append(torch.full((H, W), 7, dtype=torch.int32, device="cuda"))
    return R.Framebuffer(ctx, W, H, dev[0].data_ptr(), dev[5].data_ptr()), arrays and R.FeatureBuffers.wrap(ctx, *dev[1:4]), R.Moments.wrap(ctx, dev[4]), dev


def filtered(ctx, arrays, params, routes=((-1, -1), (0, 0), (1, 0), (0, 1), (1, 1))):
    import raytracerwin_amd as R
    H, W = arrays[0].shape[:2]
    src, feat, mom, dev = wrapped(ctx, arrays[:4], arrays[4])
    dst = wrapped(ctx, None, arrays[4])[0]
    p = R.DenoiseVarianceParams(levels=params[0], sigma_lum=params[1], sigma_normal=params[2], sigma_depth=params[3], flags=params[4], min_history=params[5])
    got = []
    for tiling, route in routes:
        ctx.set_option("denoise_tiling", tiling), ctx.set_option("variance_prefilter", route)
        R.denoise_variance(src, feat, mom, dst, p)
        got.append((dst.read_float().reshape(H, W, 4), dst.resolve_argb()))
    ctx.set_option("denoise_tiling", -1), ctx.set_option("variance_prefilter", -1)
    return got, [d.cpu().numpy() for d in dev[:5]], (src, feat, dst)


@pytest.mark.parametrize("W,H,params", VS.CASES)
def test_variance_filter_equals_the_formula(ctx, W, H, params):
    from raytracerwin_amd import api
    arrays = VS.inputs(W, H)
    got, after, _ = filtered(ctx, arrays, params)
    accum, argb = got[0]
    err = VS.error(accum[..., :3], VS.reference(*arrays, params))
    print("error %.3e of bound %.3e" % (err, BOUND))
    assert err <= BOUND and (accum[..., 3] == 1).all()
    assert (argb == VS.pack(api.gamma_thresholds(), accum[..., :3].reshape(-1, 3))).all()
    assert all((a.view(np.uint32) == b.view(np.uint32)).all() for a, b in zip(arrays, after))
    assert all((a.view(np.uint32) == accum.view(np.uint32)).all() and (c == argb).all() for a, c in got[1:])


@pytest.mark.parametrize("W,H", [(37, 23), (131, 70)])
def test_without_sigma_lum_the_bits_are_rtw_denoise_without_sigma_color(ctx, W, H):
    import raytracerwin_amd as R
    got, _, (src, feat, dst) = filtered(ctx, VS.inputs(W, H), (5, 0.0) + VS.DEFAULTS[2:], routes=((-1, -1), (1, 1)))
    R.denoise(src, feat, dst, R.DenoiseParams(sigma_color=0.0))
    plain = dst.read_float().reshape(H, W, 4), dst.resolve_argb()
    assert all((a.view(np.uint32) == plain[0].view(np.uint32)).all() and (c == plain[1]).all() for a, c in got)


def reprojected(ctx, cams, cur, hist, m_hist, params):
    import raytracerwin_amd as R
    H, W = cur[0].shape[:2]
    (fc, tc, _, keep_c), (fh, th, mh, keep_h), (dst, _, md, keep) = wrapped(ctx, cur, m_hist), wrapped(ctx, hist, m_hist), wrapped(ctx, None, m_hist)
    p, cams = R.ReprojectParams(depth_tolerance=params[0], normal_cos=params[1], max_history=params[2], flags=params[3]), [camera(c) for c in cams]
    got = []
    for s in (-1, 0, 1):
        ctx.set_option("reproject_staging", s)
        R.reproject_moments(cams[0], cams[1], fc, tc, fh, th, mh, dst, md, p, 5)
        got.append((dst.read_float().reshape(H, W, 4), dst.resolve_argb(), md.read().reshape(H, W, 2)))
    ctx.set_option("reproject_staging", -1)
    R.reproject(cams[0], cams[1], fc, tc, fh, th, dst, p)
    return got, (dst.read_float().reshape(H, W, 4), dst.resolve_argb()), (fc, tc, fh, th, mh, dst, md, keep, keep_c, keep_h)


@pytest.mark.parametrize("W,H,pair,params", RS.CASES)
def test_reprojected_moments_equal_the_formula(ctx, W, H, pair, params):
    cc, cp, cleared = RS.PAIRS[pair]
    cur, hist = RS.inputs(W, H, cc, cp, cleared)
    m_hist = VS.history_moments(hist)
    got, plain, _ = reprojected(ctx, (cc, cp), cur, hist, m_hist, params)
    ref, ref_n, margin = VS.moments_reference(cc, cp, cur, hist, m_hist, params, 5)
    compared, share = RS.excluded(margin, cur)
    err = VS.moments_error(got[0][2], ref, compared)
    print("error %.3e of bound %.3e, excluded %.4f" % (err, BOUND_MOMENTS, share))
    assert share <= 0.03 and err <= BOUND_MOMENTS
    for accum, argb, mu in got:
        assert (accum.view(np.uint32) == plain[0].view(np.uint32)).all() and (argb == plain[1]).all() and (mu.view(np.uint32) == got[0][2].view(np.uint32)).all()


def test_an_unmoved_camera_accumulates_the_moments_exactly(ctx):
    """three calls from cleared buffers, the current frame brightened each time: mu_k = mu_{k-1} + ((l, l * l) - mu_{k-1}) / k in float32"""
    import torch
    import raytracerwin_amd as R
    W, H, f32 = 37, 23, np.float32
    cur, hist = RS.inputs(W, H, RS.HOME, RS.HOME)
    (fc, tc, _, keep_c), (_, th, _, keep_h) = wrapped(ctx, cur, np.zeros((H, W, 2), f32)), wrapped(ctx, hist, np.zeros((H, W, 2), f32))
    ping, mom = [R.Framebuffer(ctx, W, H), R.Framebuffer(ctx, W, H)], [R.Moments(ctx, W, H), R.Moments(ctx, W, H)]
    ping[0].clear()
    good, want, cam = np.isfinite(cur[0][..., :3]).all(-1), np.zeros((H, W, 2), f32), camera(RS.HOME)
    for k in range(3):
        scaled = cur[0].copy()
        scaled[..., :3] *= f32(k + 1)
        keep_c[0].copy_(torch.from_numpy(scaled))
        R.reproject_moments(cam, cam, fc, tc, ping[k & 1], th, mom[k & 1], ping[(k + 1) & 1], mom[(k + 1) & 1], R.ReprojectParams(depth_tolerance=0.0, normal_cos=-1.0, flags=0), 5)
        l = VS.lum(scaled[..., :3] / f32(2), f32)
        sample = np.stack([l, l * l], -1)
        want = sample if k == 0 else want + (sample - want) / f32(k + 1)
    got = mom[1].read().reshape(H, W, 2)
    assert good.sum() > W * H // 2 and (got[good].view(np.uint32) == want[good].astype(f32).view(np.uint32)).all()
    assert (ping[1].read_float().reshape(H, W, 4)[..., 3][good] == 3).all()


def test_refusals_leave_both_destinations_alone(ctx):
    import raytracerwin_amd as R
    cur, hist = RS.inputs(16, 8, RS.HOME, RS.HOME)
    _, _, (fc, tc, fh, th, mh, dst, md, keep, _, _) = reprojected(ctx, (RS.HOME, RS.HOME), cur, hist, VS.history_moments(hist), RS.DEFAULTS)
    keep = [t.fill_(7) for t in (keep[0], keep[4], keep[5])]
    other, cam = R.Context(0), camera(RS.HOME)
    rp = [(mh, dst, mh, {}, 5), (None, dst, md, {}, 5), (mh, dst, None, {}, 5), (R.Moments(ctx, 17, 8), dst, md, {}, 5), (mh, dst, R.Moments(other, 16, 8), {}, 5),
          (mh, dst, md, {}, 0), (mh, dst, md, {}, 65536), (mh, dst, md, dict(max_history=0), 5), (mh, fh, md, {}, 5)]
    for m_hist, d, m_dst, kw, history in rp:
        with pytest.raises((R.RtwError, AttributeError)):
            R.reproject_moments(cam, cam, fc, tc, fh, th, m_hist, d, m_dst, R.ReprojectParams(**kw), history)
    dv = [(fc, tc, None, dst, {}), (fc, tc, R.Moments(ctx, 16, 9), dst, {}), (fc, tc, R.Moments(other, 16, 8), dst, {}), (fc, tc, mh, fc, {}),
          (fc, tc, mh, dst, dict(min_history=0)), (fc, tc, mh, dst, dict(min_history=65)), (fc, tc, mh, dst, dict(levels=7)), (fc, tc, mh, dst, dict(sigma_lum=float("nan")))]
    for s, f, m, d, kw in dv:
        with pytest.raises((R.RtwError, AttributeError)):
            R.denoise_variance(s, f, m, d, R.DenoiseVarianceParams(**kw))
    ctx.synchronize()
    assert all((t.cpu().numpy() == 7).all() for t in keep)
    other.close()
