"""rtw_denoise on the GPU over wrapped torch tensors against the float64 NumPy evaluation of include/rtwin.h's formula (tests/denoise_support.py):
the value, the count, the exact gamma pack, untouched sources, and the two tilings bit for bit."""
import numpy as np
import pytest

import denoise_support as DS

pytestmark = pytest.mark.gpu
D = DS.DEFAULTS
# 8 x the largest error of the float32 NumPy evaluation against the float64 one over all these cases (2.132e-07: profiles/denoise_experiments.md section 1)
BOUND = 1.706e-06
FRAMES = [(1, 1), (5, 3), (37, 23), (131, 70), (300, 33)]
PARAMS = [(5, 0.6, 0, 0, 0), (5, 0, 0.3, 0, 0), (5, 0, 0, 0.1, 0), (1,) + D[1:], (6,) + D[1:], D[:4] + (DS.DEMODULATE,), D[:4] + (DS.SAME_SHAPE,)]
CASES = [(W, H, D) for W, H in FRAMES] + [(37, 23, p) for p in PARAMS]


@pytest.fixture(scope="module")
def ctx():
    import torch
    import raytracerwin_amd as R
    torch.cuda.init()
    c = R.Context(0, stream=torch.cuda.current_stream().cuda_stream)       # the wrapped tensors are written on torch's stream
    yield c
    c.close()


def run(ctx, arrays, params, tilings=(-1, 0, 1)):
    """[(accum (H, W, 4) with the count as a float, argb (H * W,)) per tiling] and the device copies of the inputs afterwards"""
    import torch
    import raytracerwin_amd as R
    H, W = arrays[0].shape[:2]
    dev = [torch.from_numpy(a).cuda() for a in arrays]
    out_a, out_c = torch.full((H, W, 4), 7.0, device="cuda"), torch.full((H, W), 7, dtype=torch.int32, device="cuda")
    src_c = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    src, dst = R.Framebuffer(ctx, W, H, dev[0].data_ptr(), src_c.data_ptr()), R.Framebuffer(ctx, W, H, out_a.data_ptr(), out_c.data_ptr())
    feat = R.FeatureBuffers.wrap(ctx, dev[1], dev[2], dev[3])
    p = R.DenoiseParams(levels=params[0], sigma_color=params[1], sigma_normal=params[2], sigma_depth=params[3], flags=params[4])
    got = []
    for t in tilings:
        ctx.set_option("denoise_tiling", t)
        R.denoise(src, feat, dst, p)
        got.append((dst.read_float().reshape(H, W, 4), dst.resolve_argb()))
    ctx.set_option("denoise_tiling", -1)
    return got, [d.cpu().numpy() for d in dev], (src, dst, feat, out_a)


def check(ctx, arrays, params):
    from raytracerwin_amd import api
    got, after, _ = run(ctx, arrays, params)
    ref = DS.reference(*arrays, params)
    accum, argb = got[0]
    err = DS.error(accum[..., :3], ref)
    print("error %.3e of bound %.3e" % (err, BOUND))
    assert err <= BOUND
    assert (accum[..., 3] == 1).all()
    assert (argb == DS.pack(api.gamma_thresholds(), accum[..., :3].reshape(-1, 3))).all()
    for a, b in zip(arrays, after):
        assert (a.view(np.uint32) == b.view(np.uint32)).all()
    for a, c in got[1:]:
        assert (a.view(np.uint32) == accum.view(np.uint32)).all() and (c == argb).all()


@pytest.mark.parametrize("W,H,params", CASES, ids=lambda v: "-".join("%g" % x for x in v) if isinstance(v, tuple) else str(v))
def test_denoise_equals_the_formula(ctx, W, H, params):
    check(ctx, DS.inputs(W, H), params)


def test_denoise_of_a_rendered_frame(ctx):
    import raytracerwin_amd as R
    from conftest import asset
    W, H = 96, 54
    s = R.RayTracerScene(ctx)
    s.AddShape(R.RMeshShape.Create(asset("TorusKnot.obj")), R.SurfaceMaterial_Diffuse((0.9, 0.6, 0.3)))
    fb, feat = R.Framebuffer(ctx, W, H), R.FeatureBuffers(ctx, W, H)
    s.render_passes(fb, 10, 0, 1, 4, R.RenderOption(False), 0, 1, 1, 12345)
    s.render_features(feat, 10, 0, 1, 0, 1, 1, 12345)
    accum = fb.read_float().reshape(H, W, 4)
    accum[..., 3] = accum[..., 3].astype(np.int32).view(np.float32)          # back to the device's layout: the counts as int bits
    geom, albedo, ids = (a.reshape(H, W, -1) for a in feat.read())
    albedo[..., 3] = albedo[..., 3].astype(np.int32).view(np.float32)
    assert len(np.unique(ids[..., 0])) == 2
    check(ctx, (accum, geom, albedo, ids), D)


def test_refusals_leave_the_destination_alone(ctx):
    import raytracerwin_amd as R
    arrays = DS.inputs(16, 8)
    _, _, (src, dst, feat, out_a) = run(ctx, arrays, D, tilings=())
    other = R.Context(0)
    bad = [(None, feat, dst, {}), (src, feat, src, {}), (src, feat, R.Framebuffer(ctx, 17, 8), {}), (src, R.FeatureBuffers(ctx, 16, 9), dst, {}),
           (R.Framebuffer(other, 16, 8), feat, dst, {}), (src, feat, dst, dict(levels=0)), (src, feat, dst, dict(levels=7)),
           (src, feat, dst, dict(sigma_depth=float("nan"))), (src, feat, dst, dict(flags=8))]
    for s, f, d, kw in bad:
        with pytest.raises((R.RtwError, AttributeError)):
            R.denoise(s, f, d, R.DenoiseParams(**kw))
    ctx.synchronize()
    assert (out_a.cpu().numpy() == 7.0).all()
    other.close()
