"""Edge cases of the leaf operations every pipeline shares, on the GPU, bit for bit: (1) rays aimed at the analytic shapes' tangents, surfaces,
segment ends, seams and axes against the reference's records and the oracle; (2) textures of awkward shapes (1 x 1, 1 x 9, 7 x 1, 5 x 3, 33 x 17; RGB and
RGBA) from files and from the caller's arrays; (3) the resolve (accumulate, mean, gamma staircase, pack) on accumulators chosen to sit on the staircase's
steps, put in front of every pipeline's resolve through wrapped torch buffers."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, asset

pytestmark = pytest.mark.gpu

import raytracerwin_amd as R  # noqa: E402
from raytracerwin_amd import api  # noqa: E402
import camera_support as CS  # noqa: E402
import scenes as SC  # noqa: E402
from oracle import oracle as _O  # noqa: E402  (material node arrays only)
from tests.golden.make_golden import EDGE_FAMILIES, ODDTEX, make_edge_rays, oddtex_texels  # noqa: E402

torch = pytest.importorskip("torch")
f32 = np.float32
ODDTEX_OBJ = os.path.join(GOLDEN, "oddtex", "oddtex.obj")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    """bit-identical, except that any NaN equals any NaN (payload/sign of a NaN is not specified)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.fixture(scope="module")
def ctx():
    c = R.Context(0, stream=torch.cuda.current_stream().cuda_stream)      # queries and renders run on torch's current stream
    yield c
    c.close()


def product_scene(ctx, shapes, camera=None):
    s = R.RayTracerScene(ctx)
    for sh in shapes:
        mat = None if sh[-1] is None else R.material_nodes_from_array(_O.materials(sh[-1]))
        mk = {"sphere": lambda: R.RSphere.Create(sh[1], sh[2]), "plane": lambda: R.RPlane.Create(sh[1], sh[2]), "capsule": lambda: R.RCapsule.Create(sh[1], sh[2], sh[3]),
              "triangle": lambda: R.RTriangle.Create(sh[1], sh[2], sh[3]), "mesh": lambda: R.RMeshShape.Create(asset(sh[1] + ".obj"))}
        s.AddShape(mk[sh[0]](), mat)
    if camera is not None:
        s.set_camera(camera)
    s.commit()
    return s


# ---- 1. rays aimed at the edges of the analytic shapes -------------------------------------------------------------------------------------
def query(ctx, s, rays_t, qk, qb, prune):
    ctx.set_option("query_kernel", qk)
    ctx.set_option("query_blocks", qb)
    s.set_prune(prune)
    try:
        hits, shape, tri = s.trace_closest(rays_t)
        occ = s.trace_occluded(rays_t)
        torch.cuda.synchronize()
    finally:
        ctx.set_option("query_kernel", -1)
        ctx.set_option("query_blocks", 0)
        s.set_prune(1)
    return hits.cpu().numpy(), shape.cpu().numpy(), tri.cpu().numpy(), occ.cpu().numpy()


def check_records(got_hits, got_shape, want_hits, want_shape, family, what):
    for f, name in enumerate(EDGE_FAMILIES):         # family by family, for the message
        m = family == f
        bad = np.flatnonzero(m & (got_shape != want_shape))
        assert len(bad) == 0, (what, name, "rays", bad[:8].tolist(), "got", got_shape[bad[:8]].tolist(), "want", want_shape[bad[:8]].tolist())
        hit = m & (want_shape >= 0)
        assert same(got_hits[hit], want_hits[hit]), (what, name)


def run_edge_rays(ctx, s, rays, family, want_hits, want_shape, prune):
    s.set_prune(prune)
    hits, shape, _ = s.FindIntersectionWithScene(rays)                 # the host path
    s.set_prune(1)
    check_records(hits, shape, want_hits, want_shape, family, "host arrays")
    rays_t = torch.from_numpy(np.ascontiguousarray(rays, np.float32)).cuda()
    for qb in (0, 2):
        new = query(ctx, s, rays_t, 1, qb, prune)
        check_records(new[0], new[1], want_hits, want_shape, family, ("query_kernel 1", qb))
        assert (new[3] == (want_shape >= 0).astype(np.uint8)).all(), ("occluded", qb)
        old = query(ctx, s, rays_t, 0, qb, prune)
        for a, b in zip(new, old):
            assert a.tobytes() == b.tobytes(), ("the two kernels differ", qb)


@pytest.mark.parametrize("prune", [0, 1])
def test_edge_rays_equal_the_reference(ctx, prune):
    """FindIntersectionWithScene (host arrays) and trace_closest / trace_occluded (device buffers, both kernels, the default grid and two blocks) over
    every ray of sceneclosest_edges.npz: the reference's shape for every ray, its record for every hit (NaN == NaN: hits whose records hold NaN
    exist), the two kernels equal byte for byte, any-hit == `shape >= 0`.

    Ray 2718 (family "odd": distance 0, origin (0.3, -3, 0.2), heading down) is the one that found a product bug.  The huge sphere's test divides
    0 by 0 for a segment of length 0 and reports a hit at distance NaN, as the reference's does; the mesh is then tested with a segment length of
    NaN, and the reference accepts a triangle through comparisons that are all false (shape 5).  The pruned walks' segment clip skipped that
    triangle's box as lying behind the origin; it is now applied only while the segment length is a number it holds for (`seg_clips`)."""
    g = np.load(os.path.join(GOLDEN, "sceneclosest_edges.npz"))
    s = product_scene(ctx, SC.SCENES["edges"]())
    try:
        run_edge_rays(ctx, s, g["rays"], g["family"], g["hit"], g["shape"], prune)
    finally:
        s.close()


@pytest.mark.parametrize("prune", [0, 1])
def test_fresh_edge_rays_equal_the_oracle(ctx, oracle_mod, prune):
    """another draw of make_edge_rays, against the oracle -- over the scene with the sphere of negative radius appended, which the reference
    itself refuses (an assertion on the shape's inverted box) and no fixture holds."""
    shapes = SC.SCENES["edges_negative"]()
    rays, family, target = make_edge_rays(shapes, np.random.default_rng(99))
    assert len(rays) <= 4000 and (target == len(shapes) - 1).any()
    hf, hs, _ = oracle_mod.Scene().add_shapes(shapes, lambda n: asset(n + ".obj")).trace_closest(rays)
    assert (hs == len(shapes) - 1).any()          # the oracle sees the sphere through the square of its radius
    s = product_scene(ctx, shapes)
    try:
        run_edge_rays(ctx, s, rays, family, hf, hs, prune)
    finally:
        s.close()


@pytest.mark.parametrize("pose", [None, "offaxis"])
def test_edges_scene_frame_equals_the_oracle(ctx, oracle_mod, pose):
    """a tiny frame of the scene (64 x 48, 2 sub-samples, depth 4, 2 passes) from the default camera (the oracle's own frame loop) and from a
    look-at pose (the oracle's explicit-ray entry behind the camera model of tests/camera_support.py), through pipelines 4, 3 and 0"""
    W, H, ns, depth, seed = 64, 48, 2, 4, 4711
    shapes = SC.SCENES["edges"]()
    if pose is None:
        ofb = oracle_mod.Framebuffer(W, H)
        os_ = oracle_mod.Scene().add_shapes(shapes, lambda n: asset(n + ".obj"))
        for p in range(2):
            os_.render_range(ofb, 0, W * H - 1, depth, False, p, ns, seed)
        want = ofb.read()
    else:
        want = CS.oracle_frame(oracle_mod, asset, shapes, CS.cam13(R, pose), W, H, ns, depth, n_passes=2, seed=seed)
    s = product_scene(ctx, shapes, CS.camera_of(R, pose))
    try:
        for pl in (4, 3, 0):
            ctx.set_option("pipeline", pl)
            fb = R.Framebuffer(ctx, W, H)
            fb.clear()
            s.render_passes(fb, 10, 0, 1, depth, None, 0, 2, ns, seed)
            a, b = fb.read_float(), fb.resolve_argb()
            fb.close()
            assert (bits(a) == bits(want[0])).all() and (b == want[1]).all(), pl
        assert len(np.unique(want[1])) > 50
    finally:
        ctx.set_option("pipeline", 4)
        s.close()


# ---- 2. textures of awkward shapes -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oddtex_scene(ctx):
    s = R.RayTracerScene(ctx)
    s.AddShape(R.RMeshShape.Create(ODDTEX_OBJ), R.SurfaceMaterial_Diffuse((1, 1, 1)))
    s.commit()
    yield s
    s.close()


@pytest.mark.parametrize("k", range(len(ODDTEX)))
def test_texture_sample_of_awkward_sizes_equals_the_reference(oddtex_scene, k):
    g = np.load(os.path.join(GOLDEN, "texsample_oddtex_m%d.npz" % k))
    assert (bits(oddtex_scene.texture_sample(0, k, g["uv"])) == bits(g["rgba"])).all()


def test_textures_handed_over_by_the_caller(ctx, oracle_mod):
    """RMeshShape.FromArrays(..., matid=..., textures={k: px}) -> rtw_scene_set_texture: the same texel arrays from the caller's memory, against the
    oracle fed through Scene.set_texture (and so against the reference's samples); NaN and inf uv only have to be survived"""
    os_ = oracle_mod.Scene()
    sh = os_.add_mesh_obj(ODDTEX_OBJ, load_textures=False)
    m = os_.mesh_arrays(sh)
    px = {k: oddtex_texels(k) for k in range(len(ODDTEX))}
    for k in px:
        os_.set_texture(sh, k, px[k])
    s = R.RayTracerScene(ctx)
    s.AddShape(R.RMeshShape.FromArrays(m["points"], m["texcoords"], m["normals"], m["pidx"], m["tidx"], m["nidx"], matid=m["matid"], textures=px),
               R.SurfaceMaterial_Diffuse((1, 1, 1)))
    s.commit()
    try:
        for k in px:
            g = np.load(os.path.join(GOLDEN, "texsample_oddtex_m%d.npz" % k))
            got = s.texture_sample(0, k, g["uv"])
            assert (bits(got) == bits(os_.texture_sample(sh, k, g["uv"]))).all() and (bits(got) == bits(g["rgba"])).all(), k
            bad = g["uv"][:12].copy()
            bad[0::4, 0] = np.nan; bad[1::4, 1] = np.inf; bad[2::4, 0] = -np.inf; bad[3::4] = np.nan
            assert s.texture_sample(0, k, bad).shape == (12, 4)
            assert (bits(s.texture_sample(0, k, g["uv"])) == bits(g["rgba"])).all()        # and the scene still answers
    finally:
        s.close()


@pytest.mark.parametrize("preview", [0, 1])
def test_oddtex_frame_equals_the_oracle(ctx, oracle_mod, oddtex_scene, preview):
    """the shading block's `tu, 1 - tv` lookup and the alpha it passes through, on the five quads: 64 x 64, 4 sub-samples, depth 2, 2 passes"""
    W, H, ns, depth, seed = 64, 64, 4, 2, 815
    os_ = oracle_mod.Scene()
    sh = os_.add_mesh_obj(ODDTEX_OBJ)
    assert os_.counts(sh)["tris"] == 2 * len(ODDTEX)
    os_.set_material(sh, [(oracle_mod.MAT_DIFFUSE, (1, 1, 1), 0, 0, 0)])
    ofb = oracle_mod.Framebuffer(W, H)
    for p in range(2):
        os_.render_range(ofb, 0, W * H - 1, depth, bool(preview), p, ns, seed)
    oa, ob = ofb.read()
    assert len(np.unique(ob)) > 100           # the quads are in view and textured
    try:
        for pl in (4, 3, 0):
            ctx.set_option("pipeline", pl)
            fb = R.Framebuffer(ctx, W, H)
            fb.clear()
            oddtex_scene.render_passes(fb, 10, 0, 1, depth, R.RenderOption(bool(preview)), 0, 2, ns, seed)
            a, b = fb.read_float(), fb.resolve_argb()
            fb.close()
            assert (b == ob).all(), pl
            if not preview:
                assert (bits(a) == bits(oa)).all(), pl
    finally:
        ctx.set_option("pipeline", 4)


# ---- 3. the resolve on chosen accumulators, through wrapped framebuffers ---------------------------------------------------------------------
RW, RH, RNS, RDEPTH, RSEED, RPASSES = 64, 48, 2, 3, 77, 3
BLACK_FROM_ROW = 30         # the black ground's rows below the mesh (the oracle's frame shows them; asserted on the device's pass colours below)
COUNTS = (0, 1, 2, 3, 1000, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1)
SPECIALS = (0.0, -0.0, -1.0, 1e-40, float(np.nextafter(f32(1), f32(0))), 1.0, 2.0, 3e38, np.inf, -np.inf)
RESOLVE_SCENE = [("mesh", "TorusKnot", SC.diffuse((0.9, 0.8, 0.7))), ("plane", (0.0, 1.0, 0.0), (0.0, -1.5, 0.0), SC.diffuse((0.0, 0.0, 0.0)))]


def step32(x, k):
    x = np.asarray(x, f32).copy()
    for _ in range(abs(k)):
        x = np.nextafter(x, f32(np.inf if k > 0 else -np.inf))
    return x


def model(pre, counts, cs):
    """AccumulatePixel::AddPixel pass by pass and GetGammaSpacePixel's mean, in float32: (sum, n, mean)"""
    with np.errstate(all="ignore"):
        s = pre.astype(f32)
        for c in cs:
            s = (s + c).astype(f32)
        n = counts.astype(np.int64) + len(cs)
        mean = (s / n.astype(f32)[:, None]).astype(f32)
    return s, n, mean


def staircase(thr, mean):
    """the words by counting thresholds (tests/test_host_cpu.py::test_gamma_threshold_staircase_equals_powf_formula); powf(-inf, 1 / 2.2f) is +inf, so a
    channel of -inf packs as 255 in the reference"""
    k = np.searchsorted(thr, mean.reshape(-1), side="right") - 1
    k = np.where(mean.reshape(-1) > 0, np.clip(k, 0, 255), np.where(mean.reshape(-1) == -np.inf, 255, 0)).astype(np.uint32).reshape(-1, 3)
    return (np.uint32(255) << 24) | (k[:, 0] << 16) | (k[:, 1] << 8) | k[:, 2]


class Wrapped:
    """accum (W * H, 4) float32 + argb int32 tensors behind rtw_framebuffer_wrap"""

    def __init__(self, ctx, accum=None, counts=None, argb=0):
        n = RW * RH
        self.accum = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        self.argb = torch.full((n,), argb, dtype=torch.int32, device="cuda")
        if accum is not None:
            self.accum[:, :3] = torch.from_numpy(accum).cuda()
            self.accum.view(torch.int32)[:, 3] = torch.from_numpy(counts.astype(np.int32)).cuda()       # the count is an int in the float's place
        torch.cuda.synchronize()
        self.fb = R.Framebuffer(ctx, RW, RH, self.accum.data_ptr(), self.argb.data_ptr())

    def read(self):
        torch.cuda.synchronize()
        a = self.accum.cpu().numpy()
        return a[:, :3].copy(), a.view(np.int32)[:, 3].astype(np.int64), self.argb.cpu().numpy().view(np.uint32)

    def close(self):
        self.fb.close()


@pytest.fixture(scope="module")
def resolve_setup(ctx, oracle_mod):
    """the scene, the device's pass colours (each pass alone into a zeroed wrapped buffer) and the preload searched from them"""
    O = oracle_mod
    s = product_scene(ctx, RESOLVE_SCENE)
    os_ = O.Scene().add_shapes(RESOLVE_SCENE, lambda n: asset(n + ".obj"))
    cs = []
    for p in range(RPASSES):
        w, own = Wrapped(ctx), R.Framebuffer(ctx, RW, RH)
        pa, pb = C.c_void_p(), C.c_void_p()
        api._check(R.library().rtw_framebuffer_device_pointers(w.fb.h, C.byref(pa), C.byref(pb)))
        assert pa.value == w.accum.data_ptr() and pb.value == w.argb.data_ptr()
        for fb in (w.fb, own):
            R.ThreadWorker_Render(s, fb, 0, RW * RH - 1, RDEPTH, None, p, RNS, RSEED)
        c, n, argb = w.read()
        assert (n == 1).all()
        assert (bits(own.read_float()[:, :3]) == bits(c)).all() and (own.resolve_argb() == argb).all()       # wrapped == library-owned
        ofb = O.Framebuffer(RW, RH)
        os_.render_range(ofb, 0, RW * RH - 1, RDEPTH, False, p, RNS, RSEED)
        assert (bits(ofb.read()[0][:, :3]) == bits(c)).all()
        w.close(); own.close()
        cs.append(c)
    black = np.arange(RW * RH) >= BLACK_FROM_ROW * RW
    for c in cs:
        assert (c[black] == 0).all()          # the preloaded value itself reaches the gamma step there
    assert sum((c[~black] != 0).any(axis=1).sum() for c in cs) > 1000
    thr = O.gamma_thresholds().astype(f32)
    yield s, cs, black, thr, build_preload(thr, cs, black)
    s.close()


def build_preload(thr, cs, black):
    """(pre (N, 3), counts (N,), target (N, 3): the step value a channel is meant to put in front of the gamma step, NaN where none, nan_channels (N, 3))"""
    rng = np.random.default_rng(31)
    N = RW * RH
    T = np.concatenate([thr, np.nextafter(thr, f32(-1)), np.nextafter(thr, f32(2))]).astype(f32)        # 3 x 256 step targets
    pre = (rng.random((N, 3), dtype=f32) * f32(4)).astype(f32)
    counts = np.zeros(N, np.int64)
    target = np.full((N, 3), np.nan, f32)
    bl, other = np.flatnonzero(black), np.flatnonzero(~black)
    extra = len(SPECIALS) + 4
    assert len(bl) >= len(T) + extra
    for i, px in enumerate(np.r_[bl[:len(T)], bl[len(T) + extra:]]):        # count 0 on the black pixels: every channel in turn gets every target
        for ch in range(3):
            pre[px, ch] = target[px, ch] = T[(i + 256 * ch) % len(T)]
    for i, px in enumerate(bl[len(T):len(T) + len(SPECIALS)]):
        pre[px] = [f32(SPECIALS[(i + ch) % len(SPECIALS)]) for ch in range(3)]
    for i, px in enumerate(bl[len(T) + len(SPECIALS):len(T) + extra]):      # a NaN in one channel, step values beside it
        pre[px] = [T[5 * i + 300], T[5 * i + 40], T[5 * i + 700]]
        pre[px, i % 3] = np.nan
    # elsewhere: random sums, counts from COUNTS; for counts > 0 a sum searched so that the mean after RPASSES passes lands on a target
    j = np.arange(len(other))
    counts[other] = np.array(COUNTS)[(j + j // len(T)) % len(COUNTS)]
    nf = (counts[other] + RPASSES).astype(f32)
    with np.errstate(all="ignore"):
        for ch in range(3):
            t = T[(j + 256 * ch) % len(T)]
            want = np.full(len(other), np.nan, f32)                          # the sum whose mean is the target
            s0 = (t.astype(np.float64) * nf.astype(np.float64)).astype(f32)
            for ds in (0, 1, -1, 2, -2):
                cand = step32(s0, ds)
                ok = np.isnan(want) & ((cand / nf).astype(f32) == t)
                want[ok] = cand[ok]
            c0, c1, c2 = (c[other, ch] for c in cs)
            p0 = (want.astype(np.float64) - c2 - c1 - c0).astype(f32)
            found = np.zeros(len(other), bool)
            for dp in (0, 1, -1, 2, -2, 3, -3):
                cand = step32(p0, dp)
                ok = ~found & ((((cand + c0).astype(f32) + c1).astype(f32) + c2).astype(f32) == want) & (counts[other] > 0)
                pre[other[ok], ch] = cand[ok]
                found |= ok
            target[other, ch] = np.where(counts[other] > 0, t, np.nan)
    return pre, counts, target, np.isnan(pre)


def reached(target, mean, where):
    """how many of the 3 x 256 x 3 (step value, channel) targets the model's mean reaches exactly on the pixels `where`"""
    hit = where[:, None] & (mean == target)
    return len({(ch, v) for ch in range(3) for v in bits(target[hit[:, ch], ch]).tolist()})


def expected(O, thr, pre, counts, cs, nan_channels):
    s, n, mean = model(pre, counts, cs)
    argb = O.make_pixel_colors(mean)
    mask = np.uint32(0xFF000000) | np.where(nan_channels[:, 0], 0, 0xFF0000).astype(np.uint32) | np.where(nan_channels[:, 1], 0, 0xFF00).astype(np.uint32) | \
        np.where(nan_channels[:, 2], 0, 0xFF).astype(np.uint32)
    assert ((argb & mask) == (staircase(thr, mean) & mask)).all()          # the two references agree
    return s, n, argb, mask


def check_state(w, want, pixels=None, what=""):
    s, n, argb, mask = want
    gs, gn, gargb = w.read()
    sel = slice(None) if pixels is None else pixels
    assert same(gs[sel], s[sel]), (what, "accumulated sums")
    assert (gn[sel] == n[sel]).all(), (what, "counts")
    bad = np.flatnonzero(((gargb ^ argb) & mask)[sel] != 0)
    assert len(bad) == 0, (what, "ARGB words", len(bad), [hex(v) for v in gargb[sel][bad[:4]]], [hex(v) for v in argb[sel][bad[:4]]])


def test_the_preload_sits_on_the_steps(resolve_setup):
    """a condition on the inputs, in the model: on the count-0 black pixels the value in front of the gamma step after the first pass is the preloaded
    one, and every one of the 3 x 256 x 3 targets is reached; on the searched pixels at least 90 % are reached by the mean after the last pass"""
    s, cs, black, thr, (pre, counts, target, nan_channels) = resolve_setup
    total = 3 * 256 * 3
    assert reached(target, model(pre, counts, cs[:1])[2], black) == total
    got = reached(target, model(pre, counts, cs)[2], ~black & (counts > 0))
    print("searched sums: %d of %d step targets reached exactly" % (got, total))
    assert got >= 0.9 * total
    assert set(counts[~black].tolist()) == set(COUNTS) and nan_channels.sum() == 4


RUNS = [("pipeline 0, a call per pass", 0, {}), ("pipeline 3", 3, {}), ("pipeline 4, group_max 256", 4, {"group_max": 256}), ("pipeline 4, group_max 2", 4, {"group_max": 2}),
        ("pipeline 4, two parts", 4, {"split_min": 2, "split_paths": 0, "group_parts": 2}), ("pipeline 4, three parts", 4, {"split_min": 2, "split_paths": 0, "group_parts": 3})]
DEFAULTS = {"pipeline": 4, "group_max": 256, "split_min": 8, "split_paths": 400000, "group_parts": 2}


@pytest.mark.parametrize("run", RUNS, ids=[r[0] for r in RUNS])
def test_resolve_on_chosen_accumulators(ctx, oracle_mod, resolve_setup, run):
    """Every pipeline's resolve (resolve_pixel, the group resolve, the sky kernels) adds the passes to a preloaded accumulator and packs the mean:
    accumulator bits and ARGB words equal numpy float32 + the oracle's MakePixelColor(LinearToGamma()) on every pixel -- after ONE pass from the
    preload (count 0 + 1: the preloaded step values themselves reach the gamma step on the black pixels) and, from a fresh copy, after all
    RPASSES (the searched sums' means sit on the steps).  NaN channels (the reference's result for NaN is undefined) are left out of the
    comparison of the words; their neighbours are not."""
    s, cs, black, thr, (pre, counts, target, nan_channels) = resolve_setup
    name, pipeline, options = run
    try:
        ctx.set_option("pipeline", pipeline)
        for k, v in options.items():
            ctx.set_option(k, v)
        for passes in (1, RPASSES):
            want = expected(oracle_mod, thr, pre, counts, cs[:passes], nan_channels)
            w = Wrapped(ctx, pre, counts)
            if pipeline == 0:
                for p in range(passes):
                    R.ThreadWorker_Render(s, w.fb, 0, RW * RH - 1, RDEPTH, None, p, RNS, RSEED)
            else:
                s.render_passes(w.fb, 10, 0, 1, RDEPTH, None, 0, passes, RNS, RSEED)
            check_state(w, want, None, (name, passes))
            w.close()
    finally:
        for k, v in DEFAULTS.items():
            ctx.set_option(k, v)


@pytest.mark.parametrize("pipeline", [0, 3, 4])
def test_a_range_or_rank_render_leaves_the_other_pixels_alone(ctx, oracle_mod, resolve_setup, pipeline):
    """rtw_render_range over [W + 3, 5 W - 2] and render_tasks of rank 1 of 3 with 10-row tasks (tasks 1 and 4: rows 10 - 19 and 40 - 47) into preloaded
    buffers (ARGB 0x5A5A5A5A): outside, accumulator and ARGB word keep every byte; inside, the model's pass"""
    s, cs, black, thr, (pre, counts, target, nan_channels) = resolve_setup
    want = expected(oracle_mod, thr, pre, counts, cs[:1], nan_channels)
    pix = np.arange(RW * RH)
    rows = pix // RW
    inside = {"range": (pix >= RW + 3) & (pix <= 5 * RW - 2), "rank": ((rows // 10) % 3 == 1)}
    assert inside["rank"].sum() == 18 * RW
    try:
        ctx.set_option("pipeline", pipeline)
        for kind, m in inside.items():
            w = Wrapped(ctx, pre, counts, argb=0x5A5A5A5A)
            if kind == "range":
                R.ThreadWorker_Render(s, w.fb, RW + 3, 5 * RW - 2, RDEPTH, None, 0, RNS, RSEED)
            else:
                s.render_tasks(w.fb, 10, 1, 3, RDEPTH, None, 0, RNS, RSEED)
            gs, gn, gargb = w.read()
            assert same(gs[~m], pre[~m]) and (gn[~m] == counts[~m]).all() and (gargb[~m] == 0x5A5A5A5A).all(), (kind, "outside")
            check_state(w, want, m, (kind, "inside"))
            w.close()
    finally:
        ctx.set_option("pipeline", 4)
