"""rtw_tonemap / rtw_exposure_meter on the GPU: after every step of tests/tonemap_support.py's cases the destination's accumulator and ARGB words, the
exposure's bits, the frame count and the histogram must equal the NumPy model of include/rtwin.h's formula bit for bit (every operation is an integer
one or a correctly rounded +, x, /: there is no tolerance).  The frames are wrapped torch tensors; 96 x 67 is seven blocks, so the histogram is merged
across blocks and XCDs and the last-block path is taken."""
import numpy as np
import pytest

from conftest import asset

pytestmark = pytest.mark.gpu

import raytracerwin_amd as R  # noqa: E402
import features_support as FS  # noqa: E402
import scenes as SC  # noqa: E402
import tonemap_support as TS  # noqa: E402


@pytest.fixture(scope="module")
def ctx():
    import torch
    torch.cuda.init()
    c = R.Context(0, stream=torch.cuda.current_stream().cuda_stream)       # the wrapped tensors are read and written on torch's stream
    yield c
    c.set_option("tonemap_histogram", -1); c.set_option("tonemap_blocks", 0)
    c.close()


@pytest.fixture(scope="module")
def frames():
    return TS.frames()


@pytest.mark.parametrize("case", list(TS.CASES))
def test_tonemap_equals_the_model(ctx, frames, case):
    import torch
    e = R.Exposure(ctx)
    try:
        for k, ((frame, mode, hist, blocks, kw), want) in enumerate(zip(TS.CASES[case], TS.expected(case, R.api.gamma_thresholds()))):
            W, H, acc = frames[frame]
            src_t = torch.from_numpy(acc).cuda()
            accum_t = torch.full((W * H, 4), float(TS.PATTERN[0]), dtype=torch.float32, device="cuda")
            argb_t = torch.full((W * H,), int(TS.PATTERN[1]), dtype=torch.int32, device="cuda")
            src, dst = R.Framebuffer(ctx, W, H, src_t.data_ptr(), argb_t.data_ptr()), R.Framebuffer(ctx, W, H, accum_t.data_ptr(), argb_t.data_ptr())
            ctx.set_option("tonemap_histogram", hist); ctx.set_option("tonemap_blocks", blocks)
            p = R.TonemapParams(flags=R.TonemapParams.HOLD if mode == "hold" else 0, **kw)
            if mode == "hold":
                e.set(2.5)
            if mode == "meter":
                R.meter_exposure(src, e, p)
            else:
                R.tonemap(src, src if mode == "inplace" else dst, None if mode == "null" else e, p)
            state = e.read()
            got = (src_t if mode == "inplace" else accum_t).cpu().numpy(), argb_t.cpu().numpy().view(np.uint32)
            src.close(); dst.close()
            assert TS.same(state, got[0], got[1], want), (case, k, state[:2], want[0][:3])
    finally:
        e.close()


def test_tonemap_of_a_rendered_frame(ctx, oracle_mod):
    """two passes of the default scene at 40 x 21 through ACES, metered: the model over the frame's read-back"""
    W, H = 40, 21
    s = FS.product_scene(R, oracle_mod, ctx, SC.default_scene(False), asset)
    fb, dst, e = R.Framebuffer(ctx, W, H), R.Framebuffer(ctx, W, H), R.Exposure(ctx)
    try:
        s.render_passes(fb, 10, 0, 1, 4, None, 0, 2, 4, 777)
        acc = fb.read_float()
        acc[:, 3] = acc[:, 3].astype(np.int32).view(np.float32)
        e.set(0.75)
        R.tonemap(fb, dst, e)
        accum, argb = dst.read_float(), dst.resolve_argb()
        accum[:, 3] = accum[:, 3].astype(np.int32).view(np.float32)
        state = (np.float32(0.75), True) + TS.FRESH[2:]
        want, img = TS.model(acc, state, {}, R.api.gamma_thresholds(), (np.zeros_like(acc), np.zeros(W * H, np.uint32)))
        assert TS.same(e.read(), accum, argb, (want, img[0], img[1])) and want[2] == 1 and want[3].sum() > W * H // 2
    finally:
        e.close(); dst.close(); fb.close(); s.close()


def test_tonemap_refuses_bad_arguments(ctx):
    other = R.Context(0)
    fb, small, dst, foreign, e, alien = R.Framebuffer(ctx, 40, 21), R.Framebuffer(ctx, 40, 20), R.Framebuffer(ctx, 40, 21), R.Framebuffer(other, 40, 21), R.Exposure(ctx), R.Exposure(other)
    try:
        nan = float("nan")
        bad = [dict(curve=3), dict(curve=-1), dict(key=nan), dict(white=nan), dict(adapt=nan), dict(white=0.0), dict(low_fraction=-0.1), dict(low_fraction=0.95),
               dict(high_fraction=1.5), dict(min_exposure=2.0, max_exposure=1.0), dict(adapt=1.5), dict(adapt=-0.1), dict(flags=2)]
        calls = [(fb, dst, e, R.TonemapParams(**kw)) for kw in bad] + [(small, dst, e, None), (fb, foreign, e, None), (fb, dst, alien, None)]
        for src, d, ex, p in calls:
            with pytest.raises(R.RtwError) as err:
                R.tonemap(src, d, ex, p)
            assert err.value.code == -1          # RTW_ERR_INVALID
        with pytest.raises(R.RtwError):
            R.meter_exposure(fb, e, R.TonemapParams(flags=R.TonemapParams.HOLD))
        assert (dst.read_float() == 0).all() and e.read()[:2] == (1.0, 0) and not e.read()[2].any()
    finally:
        alien.close(); e.close(); foreign.close(); dst.close(); small.close(); fb.close(); other.close()
