"""Per-pixel pass budgets on the GPU.  render_passes_budget against the uniform call: the framebuffer already holds two passes; the twelve uniform
snapshots k = 0..11 of passes 3.. are rendered into copies of it with render_passes, and pixel p of the expected frame takes snapshot
e(p) = min(max(budget[p], 0), 11).  Accumulator and ARGB are compared bit for bit at every pixel, the untouched ones (e = 0, another rank's) included.
sample_budget against a float32 NumPy evaluation of include/rtwin.h's formula, op for op: integer equality at every pixel."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import asset

pytestmark = pytest.mark.gpu

import raytracerwin_amd as R  # noqa: E402
import camera_support as CS  # noqa: E402
import scenes as SC  # noqa: E402
from oracle import oracle as _O  # noqa: E402  (material node arrays only)

W, H, FIRST, N, DEPTH, SEED = 70, 37, 3, 11, 4, 12345
DEFAULTS = {"group_max": 256, "split_paths": 400000, "primary_passes": 0}
f32 = np.float32


def budget_pattern():
    """a fixed function of the pixel: nine values over a skewed lattice, then (16 x 4 tiles) a busy tile and a sky tile at 0 and a busy tile at 11"""
    py, px = np.mgrid[0:H, 0:W]
    b = np.array([-2, 0, 1, 2, 5, 10, 11, 12, 40], np.int32)[(7 * px + 3 * py) % 9]
    b[16:20, 32:48] = 0         # the frame's centre: on the mesh
    b[0:4, 0:16] = 0            # a corner: sky
    b[16:20, 16:32] = 11
    return b


def build(ctx, name):
    shapes = {"torus": CS.TORUS, "multi": SC.default_scene(False), "lens": CS.TORUS, "lookat": CS.TORUS}[name]
    s = R.RayTracerScene(ctx)
    for sh in shapes:
        mat = R.material_nodes_from_array(_O.materials(sh[-1]))
        make = {"sphere": R.RSphere.Create, "plane": R.RPlane.Create, "capsule": R.RCapsule.Create}.get(sh[0])
        s.AddShape(make(*sh[1:-1]) if make else R.RMeshShape.Create(asset(sh[1] + ".obj")), mat)
    if name == "lookat":
        s.set_camera(CS.camera_of(R, "offaxis"))
    if name == "lens":
        s.set_lens(R.Lens(0.15, 6.5))
    s.commit()
    return s


@pytest.fixture(scope="module")
def ctx():
    c = R.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scenes(ctx):
    built = {}
    yield lambda name: built.setdefault(name, build(ctx, name))
    for s in built.values():
        s.close()


class Frame:
    """a framebuffer over torch tensors, so that a starting state can be put back"""

    def __init__(self, ctx):
        self.ctx = ctx
        self.accum = torch.zeros((H * W, 4), dtype=torch.float32, device="cuda:0")
        self.argb = torch.zeros(H * W, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        self.fb = R.Framebuffer(ctx, W, H, self.accum.data_ptr(), self.argb.data_ptr())

    def get(self):
        self.ctx.synchronize()
        return self.accum.cpu().numpy().view(np.uint32).copy(), self.argb.cpu().numpy().copy()

    def put(self, state):
        self.ctx.synchronize()
        self.accum.copy_(torch.from_numpy(state[0].view(np.float32)))
        self.argb.copy_(torch.from_numpy(state[1]))
        torch.cuda.synchronize()


_snapshots = {}


def snapshots(ctx, scene, name, ns, part):
    """(starting frame, the twelve uniform snapshots) of one scene, sub-sample count and task partition: rendered once, shared, never changed"""
    key = (name, ns, part)
    if key not in _snapshots:
        fr = Frame(ctx)
        scene.render_passes(fr.fb, 10, 0, 1, DEPTH, None, 1, 2, ns, SEED)       # every pixel holds two passes, whatever the partition below
        start = fr.get()
        snaps = []
        for k in range(N + 1):
            fr.put(start)
            scene.render_passes(fr.fb, *part, DEPTH, None, FIRST, k, ns, SEED)
            snaps.append(fr.get())
        fr.fb.close()
        _snapshots[key] = (start, snaps)
    return _snapshots[key]


def check(ctx, scenes, name, ns, options, part=(10, 0, 1)):
    scene = scenes(name)
    start, snaps = snapshots(ctx, scene, name, ns, part)
    budget = budget_pattern()
    e = np.clip(budget, 0, N).ravel()
    want_accum = np.stack([s[0] for s in snaps])[e, np.arange(H * W)]
    want_argb = np.stack([s[1] for s in snaps])[e, np.arange(H * W)]
    fr = Frame(ctx)
    fr.put(start)
    dev = torch.from_numpy(budget).to("cuda:0").contiguous()
    torch.cuda.synchronize()
    try:
        for k, v in options.items():
            ctx.set_option(k, v)
        scene.render_passes_budget(fr.fb, dev, *part, DEPTH, FIRST, N, ns, SEED)
        assert ctx.last_pass_pipeline() == 4
        accum, argb = fr.get()
    finally:
        for k, v in DEFAULTS.items():
            ctx.set_option(k, v)
        fr.fb.close()
    bad = np.flatnonzero((accum != want_accum).any(axis=1) | (argb != want_argb))
    assert bad.size == 0, (bad.size, bad[:8], e[bad[:8]])
    assert (snaps[N][0] != start[0]).any() and (want_accum != snaps[N][0]).any()       # the budget made a difference


@pytest.mark.parametrize("ns", [1, 2])
@pytest.mark.parametrize("name", ["torus", "multi", "lens", "lookat"])
def test_budgeted_passes_equal_the_uniform_snapshots(ctx, scenes, name, ns):
    check(ctx, scenes, name, ns, {})


# group_max 16 is this file's own: at 11 passes the issue's group_max 8 forms groups of 6 and 5, below split_min, and does not split; 16 forms ONE group of 11 in two parts
@pytest.mark.parametrize("options", [{"group_max": 4}, {"group_max": 8, "split_paths": 1}, {"group_max": 16, "split_paths": 1}, {"primary_passes": 2}, {"primary_passes": -1}],
                         ids=lambda o: "-".join("%s%d" % kv for kv in o.items()))
@pytest.mark.parametrize("name,ns", [("torus", 1), ("torus", 2), ("multi", 2)])
def test_groups_parts_and_ray_sets(ctx, scenes, name, ns, options):
    check(ctx, scenes, name, ns, options)


def test_another_ranks_pixels_stay(ctx, scenes):
    check(ctx, scenes, "torus", 2, {"group_max": 4}, part=(10, 1, 2))


def test_refusals(ctx, scenes):
    scene, fr, L = scenes("torus"), Frame(ctx), R.library()
    dev = torch.from_numpy(budget_pattern()).to("cuda:0")
    torch.cuda.synchronize()
    before = fr.get()

    def call(budget=dev.data_ptr(), first=FIRST, n=N):
        return L.rtw_render_passes_budget(scene.h, fr.fb.h, C.c_void_p(budget), 10, 0, 1, DEPTH, first, n, 1, C.c_uint32(SEED))
    invalid = call(budget=None)
    assert invalid < 0 and call(first=-1) == invalid and call(n=-1) == invalid
    try:
        for pipeline in (3, 0):
            ctx.set_option("pipeline", pipeline)
            assert call() == invalid
        ctx.set_option("pipeline", 4)
        ctx.stats_enable(True)
        assert call() == invalid
        ctx.stats_enable(False)
        scene.set_traversal(0)          # group_pipeline_ok is false
        assert call() == invalid
    finally:
        ctx.set_option("pipeline", 4)
        ctx.stats_enable(False)
        scene.set_traversal(1)
    after = fr.get()
    assert (after[0] == before[0]).all() and (after[1] == before[1]).all()
    assert call() == 0      # and the same arguments go through once nothing is in the way
    fr.fb.close()


# ---- sample_budget ---------------------------------------------------------------------------------------------------------------------
def budget_reference(count, mu, p):
    """include/rtwin.h's formula in float32, every operation rounded on its own"""
    mu1, mu2, n = mu[..., 0].astype(f32), mu[..., 1].astype(f32), count.astype(np.int32)
    with np.errstate(all="ignore"):
        v = np.fmax(mu2 - mu1 * mu1, f32(0))
        d = f32(p.tolerance) * (mu1 + f32(1e-3))
        x = v / (d * d) - n.astype(f32)
        b0 = np.where(~(x < f32(p.max_passes)), p.max_passes, np.where(x <= f32(p.min_passes), p.min_passes, np.ceil(np.where(np.isfinite(x), x, 0)))).astype(np.int32)
    b0 = np.where(n < p.min_history, p.max_passes, b0).astype(np.int32)
    r = p.radius
    pad = np.zeros((H + 2 * r, W + 2 * r), np.int32)
    pad[r:r + H, r:r + W] = b0
    return np.max([pad[dy:dy + H, dx:dx + W] for dy in range(2 * r + 1) for dx in range(2 * r + 1)], axis=0)


def budget_inputs():
    """counts below, at and above min_history (columns 0..2); seeded moments; rows of special values: mu2 < mu1^2, mu1 = 0, NaN, inf; and rows whose x
    lies on or within a few ulps of an integer -- of min_passes (2), of max_passes (64) and of interior ones: the float32 reference decides each, the
    kernel must agree"""
    rng = np.random.default_rng(7)
    count = rng.integers(1, 40, (H, W)).astype(np.int32)
    count[:, 0:3] = [3, 4, 5]
    mu = np.empty((H, W, 2), f32)
    mu[..., 0] = rng.random((H, W), dtype=f32)
    mu[..., 1] = mu[..., 0] * mu[..., 0] + (rng.random((H, W), dtype=f32) * f32(0.05)) ** 2
    mu[3, :, 1] = mu[3, :, 0] * mu[3, :, 0] - f32(0.01)         # mu2 < mu1^2
    mu[5, :, 0] = 0                                             # mu1 = 0
    mu[7, ::2, 0], mu[7, 1::2, 1] = np.nan, np.nan
    mu[9, ::3, 0], mu[9, 1::3, 1], mu[9, 2::3, :] = np.inf, np.inf, -np.inf
    # mu1 = 1, so d = 0.25 * 1.001f; mu2 = 1 + t * d * d, swept a few ulps either side: need = (mu2 - 1) / (d * d) lands on or beside t, and with
    # count 10, t = 12 / 74 / 30 put x at min_passes / max_passes / an interior integer (75 and 11: just outside the two ends)
    d = f32(0.25) * (f32(1) + f32(1e-3))
    dd = d * d
    for row, t in ((11, 12), (13, 74), (15, 30), (17, 75), (19, 11)):
        count[row, :] = 10
        mu[row, :, 0] = 1
        mu[row, :, 1] = f32(1) + f32(t) * dd * (f32(1) + (np.arange(W) - W // 2).astype(f32) * f32(2.0 ** -23))
    return count, mu


@pytest.mark.parametrize("radius", [0, 1, 2])
def test_sample_budget_equals_the_formula(ctx, radius):
    count, mu = budget_inputs()
    p = R.SampleBudgetParams(tolerance=0.25, min_history=4, min_passes=2, max_passes=64, radius=radius)
    want = budget_reference(count, mu, p)
    assert (want == 2).any() and (want == 64).any() and np.unique(want).size > 8
    accum = np.zeros((H, W, 4), f32)
    accum[..., 3] = count.view(f32)
    fr = Frame(ctx)
    fr.put((accum.reshape(-1, 4).view(np.uint32), np.zeros(H * W, np.int32)))
    mu_dev = torch.from_numpy(mu).to("cuda:0").contiguous()
    out = torch.full((H, W), -7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    m = R.Moments.wrap(ctx, mu_dev)
    R.sample_budget(fr.fb, m, out, p)
    ctx.synchronize()
    got = out.cpu().numpy()
    assert (got == want).all(), np.argwhere(got != want)[:8]
    L = R.library()
    for bad in (dict(tolerance=0.0), dict(tolerance=float("nan")), dict(tolerance=-1.0), dict(min_passes=-1), dict(min_passes=5, max_passes=4), dict(max_passes=65536),
                dict(min_history=0), dict(radius=-1), dict(radius=3)):
        with pytest.raises(R.RtwError):
            R.sample_budget(fr.fb, m, out, R.SampleBudgetParams(**bad))
    small = R.Moments(ctx, W - 1, H)
    with pytest.raises(R.RtwError):
        R.sample_budget(fr.fb, small, out, p)
    assert L.rtw_sample_budget(fr.fb.h, m.h, C.byref(p), None) < 0 and L.rtw_sample_budget(None, m.h, C.byref(p), C.c_void_p(out.data_ptr())) < 0
    assert L.rtw_sample_budget(fr.fb.h, m.h, None, C.c_void_p(out.data_ptr())) < 0
    ctx.synchronize()
    assert (out.cpu().numpy() == want).all()        # a refused call writes nothing
    small.close()
    m.close()
    fr.fb.close()
