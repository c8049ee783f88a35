"""The material classes of pipeline 4 on the GPU: the small scenes of tests/matclass_support.py with option "material_variants" 1 against 0 in
one process -- the accumulator's bits and the ARGB words equal (a preview frame too), pipeline 4 ran both times, and the class each call's
shade / primary kernels were instantiated for is the case's with the option on and GENERAL with it off: neither a silent fallback nor a flat
kernel where it has no business.  With the work counters on every scene runs the general kernels, and the counters do not depend on the option."""
import pytest

from conftest import asset

pytestmark = pytest.mark.gpu

import raytracerwin_amd as R  # noqa: E402
import camera_support as CS  # noqa: E402
import matclass_support as MC  # noqa: E402
from oracle import oracle as _O  # noqa: E402  (material node arrays only)


@pytest.fixture(scope="module")
def ctx():
    c = R.Context(0)
    yield c
    c.close()


def scene_of(ctx, c):
    name, mesh, tree, pose = c[:4]
    s = R.RayTracerScene(ctx)
    s.AddShape(R.RMeshShape.Create(asset(mesh + ".obj")), None if tree is None else R.material_nodes_from_array(_O.materials(tree)))
    if pose is not None:
        s.set_camera(CS.camera_of(R, pose))
    s.commit()
    return s


def render(ctx, s, c, variants, preview=False):
    """(accumulator, ARGB, class that ran) of the case's passes in one call into a cleared framebuffer"""
    w, h, n_passes, ns, depth, options = c[4:10]
    ctx.set_option("material_variants", variants)
    for k, v in dict(MC.OPTION_DEFAULTS, **options).items():
        ctx.set_option(k, v)
    fb = R.Framebuffer(ctx, w, h)
    try:
        fb.clear()
        s.render_passes(fb, 10, 0, 1, depth, R.RenderOption(preview), 0, n_passes, ns, MC.SEED)
        out = fb.read_float(), fb.resolve_argb(), ctx.last_pass_material_class()
        assert ctx.last_pass_pipeline() == 4
    finally:
        fb.close()
        ctx.set_option("material_variants", 1)
        for k, v in MC.OPTION_DEFAULTS.items():
            ctx.set_option(k, v)
    return out


def on_against_off(ctx, s, c):
    for preview in (False, True):
        a1, b1, cls1 = render(ctx, s, c, 1, preview)
        a0, b0, cls0 = render(ctx, s, c, 0, preview)
        assert cls1 == c[10] and cls0 == MC.GENERAL, (cls1, cls0, preview)
        assert (MC.bits(a1) == MC.bits(a0)).all() and (b1 == b0).all(), preview


@pytest.mark.parametrize("case", MC.CASES, ids=MC.case_id)
def test_variants_on_equal_variants_off(ctx, case):
    s = scene_of(ctx, case)
    try:
        on_against_off(ctx, s, case)
    finally:
        s.close()


def test_flat_frames_equal_the_oracle(ctx, oracle_mod):
    """the two flat classes at the base shape against the oracle itself, so that "equal to GENERAL" is anchored on this device as well"""
    for c in (MC.FLAT_CASES[0], MC.FLAT_CASES[2]):
        s = scene_of(ctx, c)
        try:
            a, b, cls = render(ctx, s, c, 1)
        finally:
            s.close()
        want = MC.oracle_frame(oracle_mod, R, asset, c)
        assert cls == c[10] and (MC.bits(a) == MC.bits(want[0])).all() and (b == want[1]).all(), c[0]


def test_class_follows_the_commit(ctx):
    """one context: a Diffuse scene (FLAT), then the same mesh committed under the Blend (GENERAL), then the Diffuse one again"""
    for c in (MC.RECOMMIT, MC.RECOMMIT_SECOND, MC.RECOMMIT):
        s = scene_of(ctx, c)
        try:
            on_against_off(ctx, s, c)
        finally:
            s.close()


def test_work_counters_do_not_depend_on_the_option(ctx):
    """stats builds keep the general kernels: the class says so, and the counters of a flat scene are the same with the option on and off"""
    c = MC.FLAT_CASES[0]
    s = scene_of(ctx, c)
    try:
        ctx.stats_enable(True)
        for _ in range(2):      # the counters are of the work AS RUN: which trace kernel a round gets hangs on the list lengths of the previous call of this shape
            render(ctx, s, c, 1)
        got = []
        for variants in (1, 0):
            ctx.stats_reset()
            a, b, cls = render(ctx, s, c, variants)
            assert cls == MC.GENERAL
            got.append((ctx.stats(), a, b))
        assert got[0][0] == got[1][0] and got[0][0]["camera_rays"] > 0 and got[0][0]["shaded_hits"] > 0
        assert (MC.bits(got[0][1]) == MC.bits(got[1][1])).all() and (got[0][2] == got[1][2]).all()
    finally:
        ctx.stats_enable(False)
        s.close()
    s = scene_of(ctx, c)
    try:
        a, b, cls = render(ctx, s, c, 1)      # counters off again: the flat kernels are back, same frame
    finally:
        s.close()
    assert cls == MC.FLAT and (MC.bits(a) == MC.bits(got[0][1])).all() and (b == got[0][2]).all()
