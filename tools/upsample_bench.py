#!/usr/bin/env python3
"""tools/upsample_bench.py CONFIG [WxH ...]  -- ON THE GPU BOX: what rtw_upsample costs and what it saves, on frames of CONFIG (bench.CONFIGS) at the
given full sizes (default 1920x1080 3840x2160), in the style of tools/variance_bench.py: HIP events on the context's stream around each set's calls,
per set 3 warm-up and 12 timed rounds, the sets interleaved twice in one session; medians.  The sets, per full size W x H:
  rtw_upsample alone from W/r x H/r, r = 2, 3, 4, under "upsample_staging" 0 and 1;
  the whole chain at W x H: render_features + reproject_moments + denoise_variance;
  the same three at W/r x H/r + render_features at W x H + upsample, r = 2, 3, 4.
The one-sample render is outside both chains (it is timed as a set of its own at each size)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import raytracerwin_amd as R  # noqa: E402
import bench  # noqa: E402

cfg = sys.argv[1]
mesh, _, _, spp, depth, kind = bench.CONFIGS[cfg]
sizes = [tuple(int(v) for v in a.split("x")) for a in sys.argv[2:]] or [(1920, 1080), (3840, 2160)]
torch.cuda.init()
ctx = R.Context(0, stream=torch.cuda.current_stream().cuda_stream)
s = R.RayTracerScene(ctx)
if kind == "setup":
    from raytracerwin_amd.setup_scene import SetupScene
    SetupScene(s, os.path.join(ROOT, "assets", mesh + ".obj"))
else:
    s.AddShape(R.RMeshShape.Create(os.path.join(ROOT, "assets", mesh + ".obj")), bench.make_material(R, kind))
s.commit()
cam = R.Camera.look_at((0.0, 0.0, 7.0), (0.0, 0.0, 0.0))
s.set_camera(cam)


class Chain:
    """the buffers of one SVGF chain at w x h, left after three frames of one camera (history length 3)"""
    def __init__(self, w, h):
        self.w, self.h = w, h
        self.sample, self.clean = R.Framebuffer(ctx, w, h), R.Framebuffer(ctx, w, h)
        self.hist, self.feat, self.mom = [R.Framebuffer(ctx, w, h) for _ in range(2)], [R.FeatureBuffers(ctx, w, h) for _ in range(2)], [R.Moments(ctx, w, h) for _ in range(2)]
        self.hist[1].clear(); self.feat[1].clear(); self.mom[1].clear()
        for k in range(3):
            self.hist.reverse(); self.feat.reverse(); self.mom.reverse()
            self.render(k)
            self.filter()

    def render(self, k=3):
        self.sample.clear()
        s.render_passes(self.sample, 10, 0, 1, depth, None, k, 1, spp, 12345)

    def filter(self):
        """render_features + reproject_moments + denoise_variance: hist[0] is the history, hist[1] the new frame"""
        s.render_features(self.feat[1], 10, 0, 1, 3, 1, spp, 12345)
        R.reproject_moments(cam, cam, self.sample, self.feat[1], self.hist[0], self.feat[0], self.mom[0], self.hist[1], self.mom[1])
        R.denoise_variance(self.hist[1], self.feat[1], self.mom[1], self.clean)


def staged(value, call):
    def run():
        ctx.set_option("upsample_staging", value)
        call()
    return run


for W, H in sizes:
    full, guide, out = Chain(W, H), R.FeatureBuffers(ctx, W, H), R.Framebuffer(ctx, W, H)
    s.render_features(guide, 10, 0, 1, 3, 1, spp, 12345)        # (an empty guide would time a kernel that takes no tap)
    sets = [("render, %dx%d" % (W, H), full.render), ("chain at %dx%d" % (W, H), full.filter)]
    for r in (2, 3, 4):
        low = Chain(W // r, H // r)
        up = lambda low=low: R.upsample(low.clean, low.feat[1], guide, out)  # noqa: E731
        sets += [("upsample x%d, staging %d" % (r, v), staged(v, up)) for v in (0, 1)]
        sets += [("render, %dx%d" % (low.w, low.h), low.render),
                 ("chain at %dx%d + features + upsample" % (low.w, low.h), staged(-1, lambda low=low, up=up: (low.filter(), s.render_features(guide, 10, 0, 1, 3, 1, spp, 12345), up())))]
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
    print("%s into %dx%d, %d spp" % (cfg, W, H, spp))
    for name, _ in sets:
        a = np.array(res[name])
        print("  %-46s median %.4f  min %.4f  (rounds %.4f / %.4f) ms per call" % (name, np.median(a), a.min(), np.median(a[:12]), np.median(a[12:])))
    del full, guide, out, sets
ctx.set_option("upsample_staging", -1)
