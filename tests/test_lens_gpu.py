"""The thin lens on the GPU, through the C ABI: frames with a lens must equal the oracle bit for bit -- its explicit-ray entry behind
the float32 lens-ray model of tests/lens_support.py -- through every pipeline and both lens routes of pipeline 4; no tolerance, no
excluded pixel.  Aperture 0 must be the pinhole exactly."""
import numpy as np
import pytest

from conftest import asset

pytestmark = pytest.mark.gpu

import raytracerwin_amd as R  # noqa: E402
import camera_support as CS  # noqa: E402
import lens_support as LS  # noqa: E402
from lens_support import bits  # noqa: E402

W, H, DEPTH, SEED, RADIUS = 96, 54, 3, 12345, 0.2
# (pipeline, lens_route): pipeline 4 through gprimary_kernel's LENS instantiation and through the camera round, pipelines 3 and 0
ROUTES = [(4, 0), (4, 1), (3, -1), (0, -1)]


@pytest.fixture(scope="module")
def ctx():
    try:                    # the device-query test hands torch tensors to the library: torch sets its GPU state up before the context exists
        import torch        # (as in tests/test_query_gpu.py, whose context is made from torch's stream)
        torch.cuda.init()
    except ImportError:
        pass
    c = R.Context(0)
    yield c
    c.close()


def lens_of(pose, radius=RADIUS):
    return R.Lens(radius, LS.target_distance(CS.POSES[pose]))


def lens2(lens):
    return (lens.aperture_radius, lens.focus_distance)


def scene_with(ctx, oracle_mod, shapes, pose, lens):
    s = CS.product_scene(R, oracle_mod, ctx, shapes, asset)
    s.set_camera(CS.camera_of(R, pose))
    s.commit()
    if lens is not None:
        s.set_lens(lens)                                   # after commit: the path that drops the cached tables
    return s


def route(ctx, pipeline, lens_route):
    ctx.set_option("pipeline", pipeline)
    ctx.set_option("lens_route", lens_route)


def frame(ctx, s, w, h, ns, first_pass=0, n_passes=1, rank_world=((0, 1),), depth=DEPTH, preview=False, calls=1):
    fb = R.Framebuffer(ctx, w, h)
    fb.clear()
    for c in range(calls):
        for rank, world in rank_world:
            s.render_passes(fb, 10, rank, world, depth, R.RenderOption(preview), first_pass + c * n_passes, n_passes, ns, SEED)
    out = fb.read_float(), fb.resolve_argb(), ctx.last_pass_pipeline()
    fb.close()
    return out


def equal(got, want):
    return bool((bits(got[0]) == bits(want[0])).all() and (got[1] == want[1]).all())


@pytest.mark.parametrize("pose", ["offaxis", "inside", "wide"])
@pytest.mark.parametrize("tag", ["torus", "mixed"])
def test_lens_frames_equal_the_oracle_through_every_pipeline(ctx, oracle_mod, tag, pose):
    shapes, cam, lens = CS.SCENES[tag], CS.cam13(R, pose), lens_of(pose)

    def want(w=W, h=H, ns=2, depth=DEPTH, **kw):
        return LS.oracle_frame(oracle_mod, asset, shapes, cam, lens2(lens), w, h, ns, depth, seed=SEED, **kw)
    s = scene_with(ctx, oracle_mod, shapes, pose, lens)
    try:
        assert s.mesh_bins(W, H, 16, 4, len(shapes) - 1) is None            # no mesh gets bins with a lens
        for pl, lr in ROUTES:
            route(ctx, pl, lr)
            got = frame(ctx, s, W, H, 2)
            assert got[2] == pl and equal(got, want()), ("one pass", pl, lr)
        for lr in (0, 1):
            route(ctx, 4, lr)
            got = frame(ctx, s, W, H, 1, 0, 5)
            assert got[2] == 4 and equal(got, want(ns=1, n_passes=5)), ("five passes in a group", lr)
            got = frame(ctx, s, W, H, 2, preview=True)
            assert equal(got, want(preview=True)), ("preview", lr)
            for depth in (0, 1):
                assert equal(frame(ctx, s, W, H, 2, depth=depth), want(depth=depth)), ("max_bounce", depth, lr)
            assert equal(frame(ctx, s, 50, 37, 2), want(50, 37)), ("a frame that does not tile", lr)
            # a pixel range that starts and ends mid-row: the pixels outside it stay cleared
            begin, end = W * 7 + 5, W * (H - 9) + 3
            fb = R.Framebuffer(ctx, W, H)
            fb.clear()
            R.ThreadWorker_Render(s, fb, begin, end, DEPTH, None, 0, 2, SEED)
            got = fb.read_float(), fb.resolve_argb()
            fb.close()
            assert ctx.last_pass_pipeline() == 4 and equal(got, want(begin=begin, end=end)), ("pixel range", lr)
        for pl in (3, 0):                                                    # the older pipelines: preview, black, a frame that falls back to pipeline 0
            route(ctx, pl, -1)
            assert equal(frame(ctx, s, W, H, 2, preview=True), want(preview=True)), ("preview", pl)
            assert equal(frame(ctx, s, W, H, 2, depth=0), want(depth=0)), ("max_bounce 0", pl)
            assert equal(frame(ctx, s, 50, 37, 2), want(50, 37)), ("50 x 37", pl)
    finally:
        route(ctx, 4, -1)
        s.close()


@pytest.mark.parametrize("lens_route", [0, 1])
def test_twenty_passes_in_one_call_equal_twenty_calls(ctx, oracle_mod, lens_route):
    lens = lens_of("offaxis")
    s = scene_with(ctx, oracle_mod, CS.MIXED, "offaxis", lens)
    try:
        route(ctx, 4, lens_route)
        once = frame(ctx, s, W, H, 1, 0, 20)
        by_one = frame(ctx, s, W, H, 1, 0, 1, calls=20)
        assert once[2] == 4 and equal(once, by_one)
        assert equal(once, LS.oracle_frame(oracle_mod, asset, CS.MIXED, CS.cam13(R, "offaxis"), lens2(lens), W, H, 1, DEPTH, n_passes=20, seed=SEED))
    finally:
        route(ctx, 4, -1)
        s.close()


def test_textured_blend_and_fuzzy_scene_pipelines_agree_with_a_lens(ctx, oracle_mod):
    """camera_support.FUZZY (texture, Blend, a fuzzy mirror): the oracle's explicit-ray entry cannot follow these (counter-stream randoms
    matter), so the pipelines and both lens routes must agree among themselves, bit for bit -- and differ from the pinhole frame"""
    s = scene_with(ctx, oracle_mod, CS.FUZZY, "offaxis", lens_of("offaxis"))
    try:
        out = {}
        for pl, lr in ROUTES:
            route(ctx, pl, lr)
            out[pl, lr] = frame(ctx, s, W, H, 2, 0, 2, depth=4)
            assert out[pl, lr][2] == pl
        assert all(equal(out[k], out[0, -1]) for k in out)
        assert len(np.unique(out[0, -1][1])) > 50                          # a picture, not a flat frame
        route(ctx, 4, -1)
        s.set_lens(None)
        assert not equal(frame(ctx, s, W, H, 2, 0, 2, depth=4), out[0, -1])
    finally:
        route(ctx, 4, -1)
        s.close()


@pytest.mark.parametrize("tag", ["torus", "mixed"])
def test_a_lens_set_and_cleared_leaves_the_pinhole_exactly(ctx, oracle_mod, tag):
    shapes = CS.SCENES[tag]
    m = len(shapes) - 1
    never = scene_with(ctx, oracle_mod, shapes, "offaxis", None)
    s = scene_with(ctx, oracle_mod, shapes, "offaxis", None)
    try:
        for pl in (4, 3, 0):
            route(ctx, pl, -1)
            want = frame(ctx, never, W, H, 2, 0, 2)
            s.set_lens(lens_of("offaxis"))
            blurred = frame(ctx, s, W, H, 2, 0, 2)
            assert s.mesh_bins(W, H, 16, 4, m) is None
            s.set_lens(R.Lens(0.0, 3.0) if pl == 3 else None)               # aperture 0 and None both mean the pinhole
            got = frame(ctx, s, W, H, 2, 0, 2)
            assert got[2] == want[2] == pl and equal(got, want) and not equal(blurred, want), pl
        (o0, e0), (o1, e1) = s.mesh_bins(W, H, 16, 4, m), never.mesh_bins(W, H, 16, 4, m)
        assert len(e0) > 0 and (o0 == o1).all() and (e0 == e1).all()         # the bins are back
        assert equal(want, CS.oracle_frame(oracle_mod, asset, shapes, CS.cam13(R, "offaxis"), W, H, 2, DEPTH, n_passes=2, seed=SEED))
    finally:
        route(ctx, 4, -1)
        never.close(); s.close()


@pytest.mark.parametrize("lens_route", [0, 1])
def test_two_ranks_compose_the_one_rank_frame(ctx, oracle_mod, lens_route):
    s = scene_with(ctx, oracle_mod, CS.MIXED, "wide", lens_of("wide"))
    try:
        route(ctx, 4, lens_route)
        fbs = []
        for rank_world in (((0, 1),), ((0, 2), (1, 2))):
            fb = R.Framebuffer(ctx, W, H)
            fb.clear()
            for rank, world in rank_world:
                s.render_tasks(fb, 10, rank, world, DEPTH, None, 0, 2, SEED)
            fbs.append((fb.read_float(), fb.resolve_argb()))
            fb.close()
        assert equal(fbs[0], fbs[1])
        assert equal(fbs[0], LS.oracle_frame(oracle_mod, asset, CS.MIXED, CS.cam13(R, "wide"), lens2(lens_of("wide")), W, H, 2, DEPTH, seed=SEED))
    finally:
        route(ctx, 4, -1)
        s.close()


@pytest.mark.parametrize("lens_route", [0, 1])
def test_reserve_sizes_the_workspace_for_every_pixel(oracle_mod, lens_route):
    """with a lens every tile is busy: rtw_render_reserve must size the workspace for all pixels, so that the render call after it
    neither falls back to smaller groups nor grows the workspace"""
    c = R.Context(0)                                                       # a context of its own: its workspace starts empty
    try:
        c.set_option("lens_route", lens_route)
        s = scene_with(c, oracle_mod, CS.TORUS, "offaxis", lens_of("offaxis"))
        fb = R.Framebuffer(c, W, H)
        fb.clear()
        s.render_reserve(fb, 10, 0, 1, DEPTH, 8, 2)
        reserved = c.workspace_bytes()
        assert reserved >= 96 * 56 * 2 * 8 * 116                             # every pixel's paths of the eight passes (116 B a slot at the least)
        s.render_passes(fb, 10, 0, 1, DEPTH, None, 0, 8, 2, SEED)
        got = fb.read_float(), fb.resolve_argb()
        assert c.fallbacks() == 0 and c.workspace_bytes() == reserved and c.last_group_passes() == 8
        assert equal(got, LS.oracle_frame(oracle_mod, asset, CS.TORUS, CS.cam13(R, "offaxis"), lens2(lens_of("offaxis")), W, H, 2, DEPTH, n_passes=8, seed=SEED))
        fb.close(); s.close()
    finally:
        c.close()


def test_device_queries_on_lens_rays_agree_with_the_frame(ctx, oracle_mod):
    """ties rtw_trace_closest_device to the host helper: a one-sample preview frame shows the sky colour of the lens ray exactly where
    the closest-hit query of R.lens_rays' ray misses"""
    torch = pytest.importorskip("torch")
    f32 = np.float32
    cam, lens = CS.camera_of(R, "offaxis"), lens_of("offaxis", 0.3)
    s = scene_with(ctx, oracle_mod, CS.TORUS, "offaxis", lens)
    try:
        rays = R.lens_rays(cam, lens, W, H, np.arange(W * H), 0, 0, SEED)
        rays_t = torch.from_numpy(rays).cuda()
        torch.cuda.synchronize()
        _, shape, _ = s.trace_closest(rays_t, hits=False, tri=False)
        ctx.synchronize()
        miss = shape.cpu().numpy() < 0
        assert 0.2 * W * H < miss.sum() < 0.98 * W * H
        argb = frame(ctx, s, W, H, 1, preview=True)[1]
        t = (f32(0.5) * (rays[:, 4] + f32(1.0))).astype(f32)               # Src/RayTracerScene.cpp:92-93
        sky = np.stack([(f32(1.0) * (f32(1.0) - t) + f32(c) * t).astype(f32) for c in (0.5, 0.7, 1.0)], 1)
        sky_argb = oracle_mod.make_pixel_colors(sky)
        assert (argb[miss] == sky_argb[miss]).all() and (argb[~miss] != sky_argb[~miss]).all()
    finally:
        s.close()
