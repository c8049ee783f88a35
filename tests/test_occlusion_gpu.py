"""rtw_render_occlusion on the GPU: the destination's accumulator and ARGB words must equal the model of tests/occlusion_support.py -- include/rtwin.h's
formula in float32 over the oracle's closest-hit query -- bit for bit at every pixel of a 40 x 21 frame (partial tiles on both edges), fed with the
features render_features left on the GPU (tested elsewhere)."""
import numpy as np
import pytest

from conftest import asset

pytestmark = pytest.mark.gpu

import raytracerwin_amd as R  # noqa: E402
import camera_support as CS  # noqa: E402
import features_support as FS  # noqa: E402
import occlusion_support as OS  # noqa: E402
import scenes as SC  # noqa: E402
from camera_support import bits  # noqa: E402

W, H, SEED = 40, 21, 777
SCENES = {"torus": CS.TORUS, "default": SC.default_scene(False), "shapes": SC.shapes_scene()}
# scene (a staged one-mesh walk / analytic shapes and a mesh / no mesh), samples, radius, flags, "occlusion_order", feature ranks (1 of 2: empty rows),
# how the two passes are called (one call / two calls), onto a framebuffer that already holds a rendered pass
CASES = [
    ("torus", 5, 0.3, 1, 0, 1, "one", False),
    ("torus", 64, 1000.0, 0, 1, 1, "one", False),
    ("torus", 1, 0.3, 1, 1, 2, "two", True),
    ("default", 5, 0.3, 1, 1, 1, "one", False),
    ("default", 1, 1000.0, 0, 0, 2, "two", False),
    ("default", 5, 1000.0, 1, 0, 1, "one", True),
    ("shapes", 64, 0.3, 1, 0, 1, "two", False),
    ("shapes", 5, 1000.0, 0, 1, 2, "one", False),
]


@pytest.fixture(scope="module")
def ctx():
    c = R.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s_s%d_r%g_f%d_o%d_w%d_%s_%s" % c)
def test_occlusion_equals_the_model(ctx, oracle_mod, case):
    tag, samples, radius, flags, order, world, calls, onto = case
    shapes = SCENES[tag]
    s = FS.product_scene(R, oracle_mod, ctx, shapes, asset)
    fb, dst = R.FeatureBuffers(ctx, W, H), R.Framebuffer(ctx, W, H)
    try:
        ctx.set_option("occlusion_order", order)
        s.render_features(fb, 4, 0, world, 0, 2, 2, SEED)
        feats = fb.read()
        assert (feats[2][:, 0] < 0).any() or tag == "shapes"                  # sky in the frame
        assert ((feats[1][:, 3] == 0).any()) == (world == 2)                  # the other rank's rows are empty
        into = None
        if onto:
            s.render_passes(dst, 10, 0, 1, 2, None, 0, 1, 4, SEED)
            into = (dst.read_float(), dst.resolve_argb())
        p = R.OcclusionParams(radius=radius, samples=samples, flags=flags)
        if calls == "one":
            s.render_occlusion(fb, dst, p, 3, 2, SEED)
        else:
            s.render_occlusion(fb, dst, p, 3, 1, SEED)
            s.render_occlusion(fb, dst, p, 4, 1, SEED)
        accum, argb = dst.read_float(), dst.resolve_argb()
        want = OS.model(R, CS.oracle_scene(oracle_mod, shapes, asset), feats, R.Camera.default().as_array(), W, H, radius, p.bias, samples, flags, 3, 2, SEED,
                        R.api.gamma_thresholds(), into)
        bad = np.flatnonzero((bits(accum) != bits(want[0])).any(axis=1) | (argb != want[1]))
        assert len(bad) == 0, (len(bad), int(bad[0]), accum[bad[0]].tolist(), want[0][bad[0]].tolist())
        if radius < 1:
            mean = accum[accum[:, 3] > 0, 0] / accum[accum[:, 3] > 0, 3]
            assert onto or ((mean < 1).any() and (mean == 1).any())           # something is occluded, something is open
    finally:
        ctx.set_option("occlusion_order", -1)
        dst.close(); fb.close(); s.close()


def test_occlusion_refuses_bad_arguments(ctx, oracle_mod):
    s = FS.product_scene(R, oracle_mod, ctx, CS.TORUS, asset)
    other = R.Context(0)
    fb, small, dst, foreign = R.FeatureBuffers(ctx, W, H), R.FeatureBuffers(ctx, W, H - 1), R.Framebuffer(ctx, W, H), R.Framebuffer(other, W, H)
    try:
        bad = [dict(samples=0), dict(samples=65), dict(radius=0.0), dict(radius=float("nan")), dict(bias=-1.0), dict(bias=float("nan")), dict(flags=2)]
        calls = [(fb, dst, R.OcclusionParams(**kw), 0, 1) for kw in bad]
        calls += [(fb, dst, None, 0, 0), (fb, dst, None, -1, 1), (fb, dst, None, (1 << 24) - 1, 2), (small, dst, None, 0, 1), (fb, foreign, None, 0, 1)]
        for f, d, p, first, n in calls:
            with pytest.raises(R.RtwError) as e:
                s.render_occlusion(f, d, p, first, n)
            assert e.value.code == -1          # RTW_ERR_INVALID
        assert (dst.read_float() == 0).all()
    finally:
        foreign.close(); dst.close(); small.close(); fb.close(); s.close(); other.close()
