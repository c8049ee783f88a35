#!/usr/bin/env python3
"""tools/budget_bench.py CONFIG [N_PASSES] [WxH]  -- ON THE GPU BOX: what per-pixel pass budgets cost and what they save, on the frame of CONFIG
(bench.CONFIGS; default 20 passes at 1920x1080), in the style of tools/upsample_bench.py: HIP events on the context's stream around each set's
call, per set 3 warm-up and 12 timed calls, the sets interleaved twice in one session; medians.  The sets:
  uniform                      render_passes, N passes
  budget, all = N              render_passes_budget with every budget N: the overhead of the BUDGET kernels (the same work)
  budget, F % of pixels        N on a seeded F % of the busy tiles' pixels, 0 elsewhere: every wave stays, the lists get shorter
  budget, F % of tiles         N on a seeded F % of the busy tiles (16 x 4 pixels), whole, 0 elsewhere: the other tiles' waves leave early as well
for F = 50, 25, 10.  A tile counts as busy here when a camera ray of one of its pixels hits a shape (render_features' ids), a little less than the
library's own list, which is by the screen bins.  Then sample_budget alone at 1920x1080 and 3840x2160 beside its traffic floor."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import raytracerwin_amd as R  # noqa: E402
import bench  # noqa: E402

cfg = sys.argv[1]
N = int(sys.argv[2]) if len(sys.argv) > 2 else 20
mesh, W, H, spp, depth, kind = bench.CONFIGS[cfg]
if len(sys.argv) > 3:
    W, H = (int(v) for v in sys.argv[3].split("x"))
torch.cuda.init()
ctx = R.Context(0, stream=torch.cuda.current_stream().cuda_stream)
s = R.RayTracerScene(ctx)
if kind == "setup":
    from raytracerwin_amd.setup_scene import SetupScene
    SetupScene(s, os.path.join(ROOT, "assets", mesh + ".obj"))
else:
    s.AddShape(R.RMeshShape.Create(os.path.join(ROOT, "assets", mesh + ".obj")), bench.make_material(R, kind))
s.commit()
fb = R.Framebuffer(ctx, W, H)
fb.clear()
s.render_reserve(fb, 10, 0, 1, depth, N, spp)

feat = R.FeatureBuffers(ctx, W, H)
feat.clear()
s.render_features(feat, 10, 0, 1, 0, 1, spp, 12345)
hit = feat.read()[2].reshape(H, W, 2)[..., 0] >= 0
TH, TW = 4, 16
pad = np.zeros(((H + TH - 1) // TH * TH, (W + TW - 1) // TW * TW), bool)
pad[:H, :W] = hit
busy_tile = pad.reshape(pad.shape[0] // TH, TH, pad.shape[1] // TW, TW).any(axis=(1, 3))
busy_pixel = np.repeat(np.repeat(busy_tile, TH, axis=0), TW, axis=1)[:H, :W]
rng = np.random.default_rng(5)


def on_device(mask):
    return torch.from_numpy(np.where(mask, N, 0).astype(np.int32)).to("cuda:0").contiguous()


budgets = [("budget, all = %d" % N, on_device(np.ones((H, W), bool)))]
for f in (50, 25, 10):
    budgets.append(("budget, %d %% of pixels" % f, on_device(busy_pixel & (rng.random((H, W)) < f / 100.0))))
    tiles = busy_tile & (rng.random(busy_tile.shape) < f / 100.0)
    budgets.append(("budget, %d %% of tiles" % f, on_device(np.repeat(np.repeat(tiles, TH, axis=0), TW, axis=1)[:H, :W])))
torch.cuda.synchronize()
sets = [("uniform", lambda: s.render_passes(fb, 10, 0, 1, depth, None, 0, N, spp, 12345))]
sets += [(name, lambda b=b: s.render_passes_budget(fb, b, 10, 0, 1, depth, 0, N, spp, 12345)) for name, b in budgets]


def measure(sets, title):
    res = {name: [] for name, _ in sets}
    for rnd in range(2):              # the sets interleaved, twice: drift of the box's clock shows as a difference between the rounds
        for name, call in sets:
            for i in range(3):
                call()
            ctx.synchronize()
            for i in range(12):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                call()
                t1.record()
                t1.synchronize()
                res[name].append(t0.elapsed_time(t1))
    print(title)
    for name, _ in sets:
        a = np.array(res[name])
        print("  %-28s median %.4f  min %.4f  (rounds %.4f / %.4f) ms per call" % (name, np.median(a), a.min(), np.median(a[:12]), np.median(a[12:])))


print("busy tiles by first hits: %d of %d (%.1f %% of the pixels)" % (busy_tile.sum(), busy_tile.size, 100.0 * busy_pixel.mean()))
measure(sets, "%s at %dx%d, %d passes of %d spp, depth %d" % (cfg, W, H, N, spp, depth))

for w, h in ((1920, 1080), (3840, 2160)):
    src, mom = R.Framebuffer(ctx, w, h), R.Moments(ctx, w, h)
    src.clear()
    mom.clear()
    out = torch.zeros((h, w), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    floor_bytes = w * h * (16 + 8 + 4)
    measure([("sample_budget, radius %d" % r, lambda r=r: R.sample_budget(src, mom, out, R.SampleBudgetParams(radius=r))) for r in (0, 1, 2)],
            "sample_budget at %dx%d: %.1f MB read and written at least (16 + 8 + 4 bytes per pixel)" % (w, h, floor_bytes / 1e6))
    src.close()
    mom.close()
