"""rtw_render_indirect on the GPU: accumulator and ARGB words must equal the model of tests/indirect_support.py (include/rtwin.h's formula in float32 over the
oracle) bit for bit at every pixel of a 40 x 21 or 37 x 21 frame (partial tiles on one edge or both), fed with the features render_features left on the GPU."""
import numpy as np
import pytest

from conftest import asset

pytestmark = pytest.mark.gpu

import raytracerwin_amd as R  # noqa: E402
import camera_support as CS  # noqa: E402
import features_support as FS  # noqa: E402
import indirect_support as IS  # noqa: E402

H, SEED = 21, 777
SCENES = {"torus": CS.TORUS, "quirk": FS.quirk_no_blend()}      # one mesh; a textured mesh with analytic shapes that carry its texel
# lights as lighting_support takes them: (type, flags, v, color, radius)
LIGHTS = {"none": [], "point": [(0, 0, (2.0, 4.0, 3.0), (1.0, 0.9, 0.8), 0.4)],
          "two": [(1, 0, (0.0, 0.8, 0.6), (0.5, 0.6, 0.7), 0.0), (0, 1, (-3.0, 3.0, 2.0), (8.0, 6.0, 4.0), 0.0)]}
LIGHTS["eight"] = LIGHTS["two"] + LIGHTS["point"] + [(0, 0, (4.0, 0.0, -3.0), (0.2, 0.2, 0.2), 0.0), (1, 0, (-0.6, 0.0, 0.8), (0.1, 0.1, 0.3), 0.05)] + LIGHTS["two"] + LIGHTS["point"]
A, M = IS.ALBEDO, IS.MIRROR
# scene, lights, samples, flags, "indirect_deal", "indirect_staging" (1: a tree's upper levels in LDS), width, two calls onto a rendered pass
CASES = [
    ("torus", "none", 1, A, 0, 0, 40, False),
    ("torus", "point", 3, A, 1, 1, 40, False),
    ("torus", "two", 1, 0, 0, 0, 37, False),
    ("torus", "two", 3, A | M, 1, 0, 40, False),
    ("torus", "point", 3, M, 0, 1, 37, True),
    ("torus", "eight", 8, A, 1, 1, 40, False),      # 64 light jobs a pixel: both mask words, the largest records
    ("quirk", "none", 3, M, 1, 0, 40, False),
    ("quirk", "point", 1, A, 0, 0, 37, False),
    ("quirk", "point", 3, 0, 1, 1, 37, False),
    ("quirk", "two", 1, M, 0, 1, 40, False),
    ("quirk", "two", 3, A, 1, 0, 37, True),
    ("quirk", "eight", 8, A, 0, 1, 37, False),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s_%s_s%d_f%d_d%d_g%d_w%d_%s" % c)
def test_indirect_equals_the_model(oracle_mod, case):
    tag, which, samples, flags, deal, staging, W, twice = case
    shapes, lights = SCENES[tag], LIGHTS[which]
    api_lights, p = [R.Light(*l) for l in lights], R.IndirectParams(samples=samples, flags=flags)
    ctx = R.Context(0)
    s = FS.product_scene(R, oracle_mod, ctx, shapes, asset)
    fb, dst = R.FeatureBuffers(ctx, W, H), R.Framebuffer(ctx, W, H)
    try:
        ctx.set_option("indirect_deal", deal)
        ctx.set_option("indirect_staging", staging)
        s.render_features(fb, 4, 0, 1, 0, 2, 2, SEED)
        into = None
        if twice:
            s.render_passes(dst, 10, 0, 1, 2, None, 0, 1, 4, SEED)
            into = (dst.read_float(), dst.resolve_argb())
            s.render_indirect(fb, dst, api_lights, p, 3, 1, SEED)
            s.render_indirect(fb, dst, api_lights, p, 4, 1, SEED)
        else:
            s.render_indirect(fb, dst, api_lights, p, 3, 2, SEED)
        accum, argb = dst.read_float(), dst.resolve_argb()
        want = IS.model(R, CS.oracle_scene(oracle_mod, shapes, asset), fb.read(), R.Camera.default().as_array(), W, H, lights, p.bias, samples, flags, 3, 2, SEED,
                        R.api.gamma_thresholds(), into)
        assert want[2] == (True,) + (bool(lights),) * 3, want[2]      # a gather miss; with lights: a lit hit, a shadowed one, a culled light job
        bad = np.flatnonzero((CS.bits(accum) != CS.bits(want[0])).any(axis=1) | (argb != want[1]))
        assert len(bad) == 0, (len(bad), int(bad[0]), accum[bad[0]].tolist(), want[0][bad[0]].tolist())
    finally:
        dst.close(); fb.close(); s.close(); ctx.close()


def test_indirect_refuses_bad_arguments(oracle_mod):
    # what differs from rtw_render_lighting's refusals (tests/test_lighting_gpu.py), and one light record the shared check refuses
    ctx = R.Context(0)
    s = FS.product_scene(R, oracle_mod, ctx, CS.TORUS, asset)
    fb, small, dst, good = R.FeatureBuffers(ctx, 40, H), R.FeatureBuffers(ctx, 40, H - 1), R.Framebuffer(ctx, 40, H), LIGHTS["point"]
    try:
        calls = [(fb, good * 9, None, 1), (fb, [(2, 0, (0.0, 0.8, 0.6), (1, 1, 1), 0.0)], None, 1), (fb, good, None, 0), (small, good, None, 1)]
        calls += [(fb, good, R.IndirectParams(**kw), 1) for kw in (dict(samples=0), dict(samples=9), dict(bias=-1.0), dict(flags=4))]
        for f, ls, p, n in calls:
            with pytest.raises(R.RtwError) as e:
                s.render_indirect(f, dst, [R.Light(*l) for l in ls], p, 0, n)
            assert e.value.code == -1          # RTW_ERR_INVALID
        assert (dst.read_float() == 0).all()
    finally:
        dst.close(); small.close(); fb.close(); s.close(); ctx.close()
