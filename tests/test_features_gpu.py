"""First-hit feature buffers on the GPU (rtw_render_features): the seven float channels, the count and the ids must equal the model of
tests/features_support.py -- the oracle's closest-hit and preview entries behind the float32 ray models -- bit for bit, no tolerance, no excluded
pixel; and the product's own ray queries and preview frames; under every option; accumulated over calls and ranks; without disturbing the renderer."""
import numpy as np
import pytest

from conftest import asset

pytestmark = pytest.mark.gpu

import raytracerwin_amd as R  # noqa: E402
import camera_support as CS  # noqa: E402
import features_support as FS  # noqa: E402
import lens_support as LS  # noqa: E402
import scenes as SC  # noqa: E402
from camera_support import bits  # noqa: E402

W, H, SEED, RADIUS = 96, 54, FS.SEED, 0.2
UNITYCHAN = [("mesh", "unitychan", SC.diffuse((1, 1, 1)))]


@pytest.fixture(scope="module")
def ctx():
    import torch
    torch.cuda.init()
    c = R.Context(0, stream=torch.cuda.current_stream().cuda_stream)       # the wrapped tensors are written on torch's stream
    yield c
    c.close()


def scene_with(ctx, oracle_mod, shapes, pose, lens=None):
    s = FS.product_scene(R, oracle_mod, ctx, shapes, asset)
    if pose is not None:
        s.set_camera(CS.camera_of(R, pose))
    s.commit()
    if lens is not None:
        s.set_lens(lens)
    return s


def lens_of(pose):
    return R.Lens(RADIUS, LS.target_distance(CS.POSES[pose]))


def lens2(lens):
    return None if lens is None else (np.float32(lens.aperture_radius), np.float32(lens.focus_distance))


def features(ctx, s, w, h, ns, first_pass=0, n_passes=1, rank_world=((0, 1),), calls=1, task_rows=10):
    fb = R.FeatureBuffers(ctx, w, h)
    for c in range(calls):
        for rank, world in rank_world:
            s.render_features(fb, task_rows, rank, world, first_pass + c * n_passes, n_passes, ns, SEED)
    out = fb.read()
    fb.close()
    return out


def check(got, want, what=""):
    assert FS.same(got, want), (what, FS.first_difference(got, want))


@pytest.mark.parametrize("pose", [None, "offaxis", "inside"])
@pytest.mark.parametrize("tag", ["torus", "mixed"])
def test_features_equal_the_model(ctx, oracle_mod, tag, pose):
    s = scene_with(ctx, oracle_mod, CS.SCENES[tag], pose)
    try:
        got = features(ctx, s, W, H, 2)
        check(got, FS.model(oracle_mod, asset, CS.SCENES[tag], CS.cam13(R, pose), None, W, H, 2))
        assert (got[2][:, 0] >= 0).any()
        if tag == "torus":
            assert (got[2][:, 0] < 0).any()                                    # hits and sky in the frame (the plane of `mixed` can fill it)
    finally:
        s.close()


@pytest.mark.parametrize("ns,n_passes", [(4, 1), (2, 2), (1, 5), (3, 3)])
def test_four_rays_per_lane_in_every_shape(ctx, oracle_mod, ns, n_passes):
    """sub-samples x passes = 4 in its three shapes, five ray sets (the fifth starts a new batch), and batches that straddle passes (3 x 3)"""
    s = scene_with(ctx, oracle_mod, CS.TORUS, "offaxis")
    try:
        assert s.mesh_bins(W, H, 16, 4, 0) is not None                        # the shared bins walk is what runs
        check(features(ctx, s, W, H, ns, 0, n_passes), FS.model(oracle_mod, asset, CS.TORUS, CS.cam13(R, "offaxis"), None, W, H, ns, n_passes=n_passes))
    finally:
        s.close()


@pytest.mark.parametrize("tag", ["torus", "mixed"])
def test_a_frame_that_does_not_tile(ctx, oracle_mod, tag):
    s = scene_with(ctx, oracle_mod, CS.SCENES[tag], "offaxis")
    try:
        check(features(ctx, s, 50, 37, 2), FS.model(oracle_mod, asset, CS.SCENES[tag], CS.cam13(R, "offaxis"), None, 50, 37, 2))
    finally:
        s.close()


def test_through_a_lens(ctx, oracle_mod):
    lens = lens_of("offaxis")
    s = scene_with(ctx, oracle_mod, CS.MIXED, "offaxis", lens)
    try:
        check(features(ctx, s, W, H, 2, 1, 2), FS.model(oracle_mod, asset, CS.MIXED, CS.cam13(R, "offaxis"), lens2(lens), W, H, 2, first_pass=1, n_passes=2))
    finally:
        s.close()


def test_textured_mesh_albedo_carries_the_sampled_colour(ctx, oracle_mod):
    s = scene_with(ctx, oracle_mod, UNITYCHAN, None)
    try:
        got = features(ctx, s, W, H, 2)
        check(got, FS.model(oracle_mod, asset, UNITYCHAN, CS.cam13(R, None), None, W, H, 2))
        hit = got[2][:, 0] >= 0
        assert len(np.unique(bits(got[1][hit, :3]), axis=0)) > 100            # texels, not one material colour
    finally:
        s.close()


def test_texel_inheritance_reaches_the_albedo(ctx, oracle_mod):
    """a sphere / capsule side in front of the textured mesh keeps the mesh hit's sampled colour (one RayHitResult serves all shapes)"""
    shapes = FS.quirk_no_blend()
    s = scene_with(ctx, oracle_mod, shapes, None)
    try:
        got = features(ctx, s, W, H, 1)
        check(got, FS.model(oracle_mod, asset, shapes, CS.cam13(R, None), None, W, H, 1))
        # the quirk is in the frame: pixels of sphere 1 (plain diffuse 0.9) whose albedo is not a grey of that material
        on_sphere = got[2][:, 0] == 1
        a = got[1][on_sphere, :3]
        assert on_sphere.any() and ((a[:, 0] != a[:, 1]) | (a[:, 1] != a[:, 2])).any()
    finally:
        s.close()


@pytest.mark.parametrize("tag,pose,lens", [("torus", None, False), ("mixed", "offaxis", True)])
def test_one_sample_equals_the_ray_queries(ctx, oracle_mod, tag, pose, lens):
    """ids and the one-sample depth / normal are what scene.trace_closest answers for rtw_lens_rays' rays"""
    import torch
    ln = lens_of(pose) if lens else None
    s = scene_with(ctx, oracle_mod, CS.SCENES[tag], pose, ln)
    try:
        geom, albedo, ids = features(ctx, s, W, H, 1, 2, 1)
        rays = R.lens_rays(CS.camera_of(R, pose) or R.Camera.default(), ln or R.Lens(0.0, 1.0), W, H, np.arange(W * H, dtype=np.int32), 2, 0, SEED)
        hits, shape, tri = s.trace_closest(torch.from_numpy(rays).cuda())
        hits, shape, tri = hits.cpu().numpy(), shape.cpu().numpy(), tri.cpu().numpy()
        miss = shape < 0
        assert (ids[:, 0] == shape).all() and (ids[:, 1] == tri).all()
        assert (bits(geom[:, 3]) == bits(np.where(miss, np.float32(1000.0), hits[:, 6]))).all()
        # (a first addend of -0 becomes +0 in the sum: the model's 0 + v)
        assert (bits(geom[:, :3]) == bits(np.where(miss[:, None], np.float32(0.0), hits[:, 3:6] + np.float32(0.0)))).all()
        assert (albedo[:, 3] == 1).all()
    finally:
        s.close()


@pytest.mark.parametrize("tag", ["default", "quirk"])
def test_one_sample_albedo_equals_the_preview_pass(ctx, oracle_mod, tag):
    """hit pixels and sky pixels: a preview frame shows GetGammaSpacePixel of the pass colour, which is the albedo (Blend draws included)"""
    shapes = SC.SCENES[tag]()
    s = scene_with(ctx, oracle_mod, shapes, None)
    try:
        geom, albedo, ids = features(ctx, s, W, H, 1, 3, 1)
        fb = R.Framebuffer(ctx, W, H)
        s.render_passes(fb, 10, 0, 1, 4, R.RenderOption(True), 3, 1, 1, SEED)
        argb = fb.resolve_argb()
        fb.close()
        assert (oracle_mod.make_pixel_colors(albedo[:, :3]) == argb).all()
        assert (ids[:, 0] >= 0).any()
        if tag == "default":
            assert (ids[:, 0] < 0).any()                                       # sky above the ground plane (quirk's plane fills the frame)
    finally:
        s.close()


def test_no_option_changes_a_bit(ctx, oracle_mod):
    want = FS.model(oracle_mod, asset, CS.MIXED, CS.cam13(R, "offaxis"), None, W, H, 2, n_passes=2)
    s = scene_with(ctx, oracle_mod, CS.MIXED, "offaxis")
    try:
        for pipeline in (0, 3, 4):
            for traversal in (0, 1):
                for prune in (0, 1):
                    ctx.set_option("pipeline", pipeline); s.set_traversal(traversal); s.set_prune(prune)
                    check(features(ctx, s, W, H, 2, 0, 2), want, (pipeline, traversal, prune))
    finally:
        ctx.set_option("pipeline", 4)
        s.close()


def test_calls_accumulate_like_passes(ctx, oracle_mod):
    want = FS.model(oracle_mod, asset, CS.TORUS, CS.cam13(R, "offaxis"), None, W, H, 2, n_passes=5)
    s = scene_with(ctx, oracle_mod, CS.TORUS, "offaxis")
    try:
        check(features(ctx, s, W, H, 2, 0, 5), want, "five passes in one call")
        check(features(ctx, s, W, H, 2, 0, 1, calls=5), want, "five calls of one pass")
        fb = R.FeatureBuffers(ctx, W, H)
        s.render_features(fb, 10, 0, 1, 0, 5, 2, SEED)
        fb.clear()
        s.render_features(fb, 10, 0, 1, 0, 5, 2, SEED)
        check(fb.read(), want, "after clear")
        depth, normal, color = fb.means()
        assert (bits(depth) == bits(want[0][:, 3] / np.float32(5))).all() and (bits(color) == bits(want[1][:, :3] / np.float32(5))).all()
        assert (bits(normal) == bits(want[0][:, :3] / np.float32(5))).all()
        fb.close()
    finally:
        s.close()


def test_ranks_share_wrapped_torch_buffers(ctx, oracle_mod):
    """FeatureBuffers.wrap over torch tensors: every rank of world 2 and 3 into the same buffers == world 1; a rank alone leaves the
    other ranks' pixels as they were; the results are read as tensors, no copy through the host by the library"""
    import torch
    want = FS.model(oracle_mod, asset, CS.MIXED, CS.cam13(R, "offaxis"), None, W, H, 2, n_passes=2)
    s = scene_with(ctx, oracle_mod, CS.MIXED, "offaxis")
    try:
        for world, rows in ((2, 10), (3, 6), (2, 3)):          # task rows of 10 / 6 / 3: 16 x 4, 32 x 2 and 64 x 1-pixel tiles
            geom = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda"); albedo = torch.zeros_like(geom)
            ids = torch.full((H, W, 2), -1, dtype=torch.int32, device="cuda")
            fb = R.FeatureBuffers.wrap(ctx, geom, albedo, ids)
            assert fb.device_pointers() == (geom.data_ptr(), albedo.data_ptr(), ids.data_ptr())
            for rank in range(world):
                s.render_features(fb, rows, rank, world, 0, 2, 2, SEED)
            count = albedo.view(torch.int32)[..., 3].clone()
            got = (geom.reshape(-1, 4).cpu().numpy(), albedo.reshape(-1, 4).cpu().numpy().copy(), ids.reshape(-1, 2).cpu().numpy())
            got[1][:, 3] = count.reshape(-1).cpu().numpy().astype(np.float32)
            check(got, want, (world, rows))
            fb.close()
        # one rank of three on top of a sentinel
        geom = torch.full((H, W, 4), 7.5, dtype=torch.float32, device="cuda"); albedo = torch.full_like(geom, -3.25)
        ids = torch.full((H, W, 2), -77, dtype=torch.int32, device="cuda")
        fb = R.FeatureBuffers.wrap(ctx, geom, albedo, ids)
        s.render_features(fb, 6, 1, 3, 0, 1, 2, SEED)
        mine = FS.share_pixels(W, H, 6, 1, 3)
        other = np.setdiff1d(np.arange(W * H), mine)
        g, a, i = geom.reshape(-1, 4).cpu().numpy(), albedo.reshape(-1, 4).cpu().numpy(), ids.reshape(-1, 2).cpu().numpy()
        assert (g[other] == 7.5).all() and (a[other] == -3.25).all() and (i[other] == -77).all()
        assert (i[mine] >= -1).all() and (bits(a[mine, 3]) != bits(np.float32(-3.25))).all()
        fb.close()
    finally:
        s.close()


def test_the_renderer_is_not_disturbed(ctx, oracle_mod):
    """a beauty frame before and after a feature call, over the same cached tile tables, is the oracle's frame"""
    want = CS.oracle_frame(oracle_mod, asset, CS.TORUS, CS.cam13(R, "offaxis"), W, H, 2, 3, n_passes=2, seed=SEED)
    s = scene_with(ctx, oracle_mod, CS.TORUS, "offaxis")
    try:
        def beauty():
            fb = R.Framebuffer(ctx, W, H)
            fb.clear()
            s.render_passes(fb, 10, 0, 1, 3, None, 0, 2, 2, SEED)
            out = fb.read_float(), fb.resolve_argb()
            fb.close()
            return out
        feat_want = FS.model(oracle_mod, asset, CS.TORUS, CS.cam13(R, "offaxis"), None, W, H, 2)
        check(features(ctx, s, W, H, 2), feat_want, "features first: they build the tables")
        a = beauty()
        assert (bits(a[0]) == bits(want[0])).all() and (a[1] == want[1]).all()
        check(features(ctx, s, W, H, 2), feat_want, "features over the renderer's tables")
        b = beauty()
        assert (bits(b[0]) == bits(want[0])).all() and (b[1] == want[1]).all()
    finally:
        s.close()


def test_camera_and_lens_changes_between_calls(ctx, oracle_mod):
    """the second call equals the model of the new pose / lens: the cached bins and tile tables were dropped"""
    s = scene_with(ctx, oracle_mod, CS.TORUS, "offaxis")
    try:
        check(features(ctx, s, W, H, 2), FS.model(oracle_mod, asset, CS.TORUS, CS.cam13(R, "offaxis"), None, W, H, 2), "first pose")
        s.set_camera(CS.camera_of(R, "below"))
        check(features(ctx, s, W, H, 2), FS.model(oracle_mod, asset, CS.TORUS, CS.cam13(R, "below"), None, W, H, 2), "second pose")
        lens = lens_of("below")
        s.set_lens(lens)
        check(features(ctx, s, W, H, 2), FS.model(oracle_mod, asset, CS.TORUS, CS.cam13(R, "below"), lens2(lens), W, H, 2), "with a lens")
        s.set_lens(None)
        check(features(ctx, s, W, H, 2), FS.model(oracle_mod, asset, CS.TORUS, CS.cam13(R, "below"), None, W, H, 2), "lens off again")
    finally:
        s.close()
