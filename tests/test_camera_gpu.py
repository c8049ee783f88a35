"""The settable camera on the GPU, through the C ABI: frames of general poses must equal the oracle bit for bit -- its explicit-ray
entry behind the float32 ray model of tests/camera_support.py -- through every pipeline and option that makes a camera ray; no
tolerance, no excluded pixel."""
import numpy as np
import pytest

from conftest import asset

pytestmark = pytest.mark.gpu

import raytracerwin_amd as R  # noqa: E402
import camera_support as CS  # noqa: E402
from camera_support import bits  # noqa: E402

DEPTH, SEED = 3, 2468
SIZES = [(192, 108), (64, 200), (100, 54)]          # 100 x 54: a frame the bins do not tile
POSE_NAMES = ["offaxis", "below", "inside", "away", "narrow", "wide"]


@pytest.fixture(scope="module")
def ctx():
    c = R.Context(0)
    yield c
    c.close()


def scene_with(ctx, oracle_mod, shapes, pose):
    s = CS.product_scene(R, oracle_mod, ctx, shapes, asset)
    cam = CS.camera_of(R, pose)
    if pose is not None:
        s.set_camera(cam)
    s.commit()
    return s


def frame(ctx, s, W, H, ns, first_pass=0, n_passes=1, rank_world=((0, 1),), depth=DEPTH):
    fb = R.Framebuffer(ctx, W, H)
    fb.clear()
    for rank, world in rank_world:
        s.render_passes(fb, 10, rank, world, depth, None, first_pass, n_passes, ns, SEED)
    out = fb.read_float(), fb.resolve_argb(), ctx.last_pass_pipeline()
    fb.close()
    return out


def equal(got, want):
    return bool((bits(got[0]) == bits(want[0])).all() and (got[1] == want[1]).all())


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("pose", POSE_NAMES)
@pytest.mark.parametrize("tag", ["torus", "mixed"])
def test_camera_frames_equal_the_oracle_through_every_pipeline(ctx, oracle_mod, tag, pose, W, H):
    shapes = CS.SCENES[tag]
    cam = CS.cam13(R, pose)
    one = CS.oracle_frame(oracle_mod, asset, shapes, cam, W, H, 2, DEPTH, n_passes=1, seed=SEED)
    five = CS.oracle_frame(oracle_mod, asset, shapes, cam, W, H, 1, DEPTH, n_passes=5, seed=SEED)
    s = scene_with(ctx, oracle_mod, shapes, pose)
    mesh_shape = len(shapes) - 1
    try:
        has_bins = s.mesh_bins(W, H, 16, 4, mesh_shape) is not None
        if pose in ("offaxis", "away"):
            assert has_bins                               # the binned path is what runs
        if pose == "inside":
            assert not has_bins
        if pose == "away" and tag == "torus":
            assert len(s.mesh_bins(W, H, 16, 4, mesh_shape)[1]) == 0      # every tile sky-only
        for pp in (0, -1, 4):
            ctx.set_option("pipeline", 4)
            ctx.set_option("primary_passes", pp)
            got = frame(ctx, s, W, H, 2)
            assert got[2] == 4 and equal(got, one), ("pipeline 4, one pass", pp)
            got = frame(ctx, s, W, H, 1, 0, 5)
            assert got[2] == 4 and equal(got, five), ("pipeline 4, five passes", pp)
        ctx.set_option("primary_passes", 0)
        tiles = W % 16 == 0 and H % 4 == 0
        for pl in (3, 0):
            ctx.set_option("pipeline", pl)
            got = frame(ctx, s, W, H, 2)
            assert got[2] == (pl if tiles else 0) and equal(got, one), ("pipeline", pl)
        ctx.set_option("pipeline", 4)
        s.set_traversal(0)
        got = frame(ctx, s, W, H, 2)
        assert got[2] == 0 and equal(got, one), "traversal 0"
        s.set_traversal(1)
        # one partial range: the pixels outside it stay cleared
        begin, end = W * 7 + 5, W * (H - 9) + 3
        fb = R.Framebuffer(ctx, W, H)
        fb.clear()
        R.ThreadWorker_Render(s, fb, begin, end, DEPTH, None, 0, 2, SEED)
        a, b = fb.read_float(), fb.resolve_argb()
        fb.close()
        assert ctx.last_pass_pipeline() == 4
        wa, wb = one[0].copy(), one[1].copy()
        wa[:begin] = 0; wa[end + 1:] = 0; wb[:begin] = 0; wb[end + 1:] = 0
        assert (bits(a) == bits(wa)).all() and (b == wb).all(), "partial range"
    finally:
        ctx.set_option("pipeline", 4)
        ctx.set_option("primary_passes", 0)
        s.close()


@pytest.mark.parametrize("pose", ["offaxis", "below"])
def test_textured_blend_and_fuzzy_scene_pipelines_agree(ctx, oracle_mod, pose):
    """a textured unitychan with Blend beside a fuzzy mirror: the oracle cannot follow these with a moved camera (counter-stream randoms
    matter), so the three pipelines must agree among themselves, bit for bit"""
    W, H = 192, 108
    s = scene_with(ctx, oracle_mod, CS.FUZZY, pose)
    try:
        out = {}
        for pl in (4, 3, 0):
            ctx.set_option("pipeline", pl)
            out[pl] = frame(ctx, s, W, H, 2, depth=4)
            assert out[pl][2] == pl
        assert equal(out[4], out[0]) and equal(out[3], out[0])
        assert len(np.unique(out[0][1])) > 50             # a picture, not a flat frame
    finally:
        ctx.set_option("pipeline", 4)
        s.close()


@pytest.mark.parametrize("tag", ["torus", "mixed"])
def test_default_pose_set_explicitly_equals_no_camera_set(ctx, oracle_mod, tag):
    W, H = 192, 108
    a, b = scene_with(ctx, oracle_mod, CS.SCENES[tag], None), scene_with(ctx, oracle_mod, CS.SCENES[tag], "default")
    try:
        assert b.get_camera() == R.Camera.default()
        for pl in (4, 3, 0):
            ctx.set_option("pipeline", pl)
            fa, fb_ = frame(ctx, a, W, H, 4, 0, 2), frame(ctx, b, W, H, 4, 0, 2)
            assert fa[2] == fb_[2] == pl and equal(fa, fb_)
        # ... and both are the oracle's own frame of its fixed camera
        ob = oracle_mod.Framebuffer(W, H)
        sc = CS.oracle_scene(oracle_mod, CS.SCENES[tag], asset)
        for p in range(2):
            sc.render_range(ob, 0, W * H - 1, DEPTH, False, p, 4, SEED)
        assert equal(fb_, ob.read())
    finally:
        ctx.set_option("pipeline", 4)
        a.close(); b.close()


@pytest.mark.parametrize("tag", ["torus", "mixed"])
def test_changing_the_pose_of_a_committed_scene_drops_the_stale_bins(ctx, oracle_mod, tag):
    W, H = 192, 108
    s = scene_with(ctx, oracle_mod, CS.SCENES[tag], "offaxis")
    fresh = scene_with(ctx, oracle_mod, CS.SCENES[tag], "below")
    try:
        for pl in (4, 3):
            ctx.set_option("pipeline", pl)
            s.set_camera(CS.camera_of(R, "offaxis"))
            first = frame(ctx, s, W, H, 2)
            s.set_camera(CS.camera_of(R, "below"))
            second = frame(ctx, s, W, H, 2)
            want = frame(ctx, fresh, W, H, 2)
            assert second[2] == want[2] == pl and equal(second, want) and not equal(second, first)
        m = len(CS.SCENES[tag]) - 1
        (o0, e0), (o1, e1) = s.mesh_bins(W, H, 16, 4, m), fresh.mesh_bins(W, H, 16, 4, m)
        assert (o0 == o1).all() and (e0 == e1).all()
        s.set_camera(None)                                # back to the default: the fixed-pose kernels, the oracle's own frame
        ob = oracle_mod.Framebuffer(W, H)
        CS.oracle_scene(oracle_mod, CS.SCENES[tag], asset).render_range(ob, 0, W * H - 1, DEPTH, False, 0, 2, SEED)
        assert equal(frame(ctx, s, W, H, 2), ob.read())
    finally:
        ctx.set_option("pipeline", 4)
        s.close(); fresh.close()


def test_two_ranks_with_the_same_camera_compose_the_one_rank_frame(ctx, oracle_mod):
    W, H = 192, 108
    s = scene_with(ctx, oracle_mod, CS.MIXED, "below")
    try:
        one = frame(ctx, s, W, H, 2, 0, 3)
        two = frame(ctx, s, W, H, 2, 0, 3, rank_world=((0, 2), (1, 2)))
        assert equal(one, two)
        assert equal(one, CS.oracle_frame(oracle_mod, asset, CS.MIXED, CS.cam13(R, "below"), W, H, 2, DEPTH, n_passes=3, seed=SEED))
    finally:
        s.close()


BINS_POSES = ["offaxis", "below", "narrow", "wide"]


@pytest.mark.parametrize("bin_w,bin_h", [(16, 4), (32, 2)])
def test_device_built_bins_equal_host_built_bins_for_general_poses(ctx, oracle_mod, bin_w, bin_h):
    """The screen bins of a mesh are the same lists whichever side built them (rtw_shared.h bins_of_leaf runs on both): exact equality of
    the offsets and the entries for general poses, a non-empty list for at least three of the four, and "no bins" from both sides for
    the pose inside the mesh's bounds."""
    W, H = 96, 54
    got = {}
    try:
        for dev in (1, 0):
            ctx.set_option("device_build", dev)
            for pose in BINS_POSES + ["inside"]:
                s = scene_with(ctx, oracle_mod, CS.TORUS, pose)
                got[dev, pose] = s.mesh_bins(W, H, bin_w, bin_h, 0)
                s.close()
    finally:
        ctx.set_option("device_build", 1)
    for pose in BINS_POSES:
        d, h = got[1, pose], got[0, pose]
        assert d is not None and h is not None, pose
        assert (d[0] == h[0]).all() and len(d[1]) == len(h[1]) and (d[1] == h[1]).all(), pose
    assert sum(1 for pose in BINS_POSES if len(got[0, pose][1]) > 0) >= 3
    assert got[1, "inside"] is None and got[0, "inside"] is None
