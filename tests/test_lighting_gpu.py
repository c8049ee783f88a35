"""rtw_render_lighting on the GPU: the destination's accumulator and ARGB words must equal the model of tests/lighting_support.py -- include/rtwin.h's
formula in float32 over the oracle's closest-hit query -- bit for bit at every pixel of a 40 x 21 frame (partial tiles on both edges), fed with the
features render_features left on the GPU (tested elsewhere)."""
import numpy as np
import pytest

from conftest import asset

pytestmark = pytest.mark.gpu

import raytracerwin_amd as R  # noqa: E402
import camera_support as CS  # noqa: E402
import features_support as FS  # noqa: E402
import lighting_support as LS  # noqa: E402
import scenes as SC  # noqa: E402
from camera_support import bits  # noqa: E402

W, H, SEED = 40, 21, 777
SCENES = {"torus": CS.TORUS, "default": SC.default_scene(False), "shapes": SC.shapes_scene()}
# lights as lighting_support takes them: (type, flags, v, color, radius)
UP = (0.0, 0.8, 0.6)
LIGHTS = {
    "one": [(0, 0, (2.0, 4.0, 3.0), (1.0, 1.0, 1.0), 0.0)],
    "two": [(0, 1, (-3.0, 3.0, 2.0), (8.0, 6.0, 4.0), 0.5), (1, 0, UP, (0.5, 0.6, 0.7), 0.1)],
    "eight": [(0, 0, (2.0, 4.0, 3.0), (0.3, 0.3, 0.3), 0.3), (1, 0, UP, (0.2, 0.1, 0.1), 0.0), (0, 1, (-3.0, 3.0, 2.0), (2.0, 2.0, 1.0), 0.0),
              (0, 0, (0.0, -4.5, 0.0), (0.1, 0.2, 0.1), 0.2), (1, 0, (-0.6, 0.0, 0.8), (0.1, 0.1, 0.3), 0.05), (0, 0, (4.0, 0.0, -3.0), (0.2, 0.2, 0.2), 0.0),
              (0, 1, (0.0, 0.5, 6.0), (3.0, 1.0, 1.0), 1.0), (1, 0, (0.0, -1.0, 0.0), (0.1, 0.1, 0.1), 0.3)],
}
# scene, lights, samples, flags (ALBEDO), "lighting_deal", feature ranks (1 of 2: empty rows), how the two passes are called (one call / two calls),
# onto a framebuffer that already holds a rendered pass
CASES = [
    ("torus", "one", 1, 1, 0, 1, "one", False),
    ("torus", "two", 3, 0, 1, 2, "two", False),
    ("torus", "eight", 8, 1, 1, 1, "one", False),
    ("default", "one", 1, 0, 1, 1, "two", True),
    ("default", "two", 3, 1, 0, 1, "one", False),
    ("default", "eight", 8, 1, 0, 2, "one", False),
    ("shapes", "two", 3, 1, 1, 1, "one", True),
    ("shapes", "eight", 8, 0, 0, 1, "two", False),
]


@pytest.fixture(scope="module")
def ctx():
    c = R.Context(0)
    yield c
    c.close()


def api_lights(lights):
    return [R.Light(t, f, v, c, r) for t, f, v, c, r in lights]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s_%s_s%d_f%d_d%d_w%d_%s_%s" % c)
def test_lighting_equals_the_model(ctx, oracle_mod, case):
    tag, which, samples, flags, deal, world, calls, onto = case
    shapes, lights = SCENES[tag], LIGHTS[which]
    s = FS.product_scene(R, oracle_mod, ctx, shapes, asset)
    fb, dst = R.FeatureBuffers(ctx, W, H), R.Framebuffer(ctx, W, H)
    try:
        ctx.set_option("lighting_deal", deal)
        s.render_features(fb, 4, 0, world, 0, 2, 2, SEED)
        feats = fb.read()
        assert ((feats[1][:, 3] == 0).any()) == (world == 2)                  # the other rank's rows are empty
        into = None
        if onto:
            s.render_passes(dst, 10, 0, 1, 2, None, 0, 1, 4, SEED)
            into = (dst.read_float(), dst.resolve_argb())
        p = R.LightingParams(samples=samples, flags=flags)
        if calls == "one":
            s.render_lighting(fb, dst, api_lights(lights), p, 3, 2, SEED)
        else:
            s.render_lighting(fb, dst, api_lights(lights), p, 3, 1, SEED)
            s.render_lighting(fb, dst, api_lights(lights), p, 4, 1, SEED)
        accum, argb = dst.read_float(), dst.resolve_argb()
        want = LS.model(R, CS.oracle_scene(oracle_mod, shapes, asset), feats, R.Camera.default().as_array(), W, H, lights, p.bias, samples, flags, 3, 2, SEED,
                        R.api.gamma_thresholds(), into)
        assert want[2] == (True, True, True), want[2]                        # something is lit, something shadowed, something culled
        bad = np.flatnonzero((bits(accum) != bits(want[0])).any(axis=1) | (argb != want[1]))
        assert len(bad) == 0, (len(bad), int(bad[0]), accum[bad[0]].tolist(), want[0][bad[0]].tolist())
    finally:
        ctx.set_option("lighting_deal", -1)
        dst.close(); fb.close(); s.close()


def test_lighting_refuses_bad_arguments(ctx, oracle_mod):
    s = FS.product_scene(R, oracle_mod, ctx, CS.TORUS, asset)
    other = R.Context(0)
    fb, small, dst, foreign = R.FeatureBuffers(ctx, W, H), R.FeatureBuffers(ctx, W, H - 1), R.Framebuffer(ctx, W, H), R.Framebuffer(other, W, H)
    good, nan = LIGHTS["one"], float("nan")
    try:
        bad_lights = [[], good * 9, [(2, 0, UP, (1, 1, 1), 0.0)], [(0, 2, UP, (1, 1, 1), 0.0)], [(0, 0, (nan, 0, 0), (1, 1, 1), 0.0)],
                      [(0, 0, UP, (1, float("inf"), 1), 0.0)], [(0, 0, UP, (1, 1, 1), nan)], [(0, 0, UP, (1, 1, 1), -0.5)],
                      [(1, 0, (0.0, 0.8, 0.7), (1, 1, 1), 0.0)], [(1, 1, UP, (1, 1, 1), 0.0)]]
        calls = [(fb, dst, ls, None, 0, 1) for ls in bad_lights]
        calls += [(fb, dst, good, R.LightingParams(**kw), 0, 1) for kw in (dict(samples=0), dict(samples=9), dict(bias=-1.0), dict(bias=nan), dict(flags=2))]
        calls += [(fb, dst, good, None, 0, 0), (fb, dst, good, None, -1, 1), (fb, dst, good, None, (1 << 24) - 1, 2), (small, dst, good, None, 0, 1),
                  (fb, foreign, good, None, 0, 1)]
        for f, d, ls, p, first, n in calls:
            with pytest.raises(R.RtwError) as e:
                s.render_lighting(f, d, api_lights(ls), p, first, n)
            assert e.value.code == -1          # RTW_ERR_INVALID
        assert (dst.read_float() == 0).all()
    finally:
        foreign.close(); dst.close(); small.close(); fb.close(); s.close(); other.close()
