#!/usr/bin/env python3
"""tools/variance_bench.py CONFIG [WxH]  -- ON THE GPU BOX: what the moments and the variance-guided filter cost beside their parents on the same
reprojected frame of CONFIG (bench.CONFIGS; WxH overrides its frame size), in the style of tools/denoise_bench.py: HIP events on the context's stream
around each call, per set 3 warm-up and 12 timed calls, the sets interleaved twice in one session.  The frame: two one-pass frames a degree apart,
reprojected (history lengths 1 and 2), or the same camera six times over (history length 6: no pixel is short of min_history 4).  The sets:
  rtw_reproject / rtw_reproject_moments under "reproject_staging" 0 and 1, moved camera;
  rtw_denoise (defaults) / rtw_denoise_variance (defaults) with "variance_prefilter" 0 (g fetched by the level kernels) and 1 (a prefilter pass);
  rtw_denoise_variance at 1 level with every pixel short of history (min_history 64) and none (min_history 1): the estimate's window, staged or not;
  "denoise_tiling" 0 / 1 with each prefilter route, 5 levels."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import raytracerwin_amd as R  # noqa: E402
import bench  # noqa: E402

cfg = sys.argv[1]
mesh, W, H, spp, depth, kind = bench.CONFIGS[cfg]
if len(sys.argv) > 2:
    W, H = (int(v) for v in sys.argv[2].split("x"))
torch.cuda.init()
ctx = R.Context(0, stream=torch.cuda.current_stream().cuda_stream)
s = R.RayTracerScene(ctx)
if kind == "setup":
    from raytracerwin_amd.setup_scene import SetupScene
    SetupScene(s, os.path.join(ROOT, "assets", mesh + ".obj"))
else:
    s.AddShape(R.RMeshShape.Create(os.path.join(ROOT, "assets", mesh + ".obj")), bench.make_material(R, kind))
s.commit()
cams = [R.Camera.look_at((7.0 * np.sin(a), 0.0, 7.0 * np.cos(a)), (0.0, 0.0, 0.0)) for a in (0.0, 0.02)]
sample, out = R.Framebuffer(ctx, W, H), R.Framebuffer(ctx, W, H)
hist, feat, mom = [R.Framebuffer(ctx, W, H) for _ in range(2)], [R.FeatureBuffers(ctx, W, H) for _ in range(2)], [R.Moments(ctx, W, H) for _ in range(3)]


def frame(k, cam, f):
    sample.clear(); f.clear()
    s.set_camera(cam)
    s.render_passes(sample, 10, 0, 1, depth, None, k, 1, spp, 12345)
    s.render_features(f, 10, 0, 1, k, 1, spp, 12345)


def fill(frames):
    """hist[1], feat[1], mom[1]: the chain after `frames` frames (the camera moves once, before the last); hist[0], feat[0], mom[0]: the frame before"""
    hist[1].clear(); feat[1].clear(); mom[1].clear()
    for k in range(frames):
        hist[0], hist[1], feat[0], feat[1], mom[0], mom[1] = hist[1], hist[0], feat[1], feat[0], mom[1], mom[0]
        frame(k, cams[1] if frames == 2 and k == 1 else cams[0], feat[1])
        R.reproject_moments(cams[1] if frames == 2 and k == 1 else cams[0], cams[0], sample, feat[1], hist[0], feat[0], mom[0], hist[1], mom[1])


def reproject_call(moments, staging):
    def call():
        ctx.set_option("reproject_staging", staging)
        if moments:
            R.reproject_moments(cams[1], cams[0], sample, feat[1], hist[0], feat[0], mom[0], out, mom[2])
        else:
            R.reproject(cams[1], cams[0], sample, feat[1], hist[0], feat[0], out)
    return call


def filter_call(tiling, route, **kw):
    params = R.DenoiseVarianceParams(**kw) if route is not None else R.DenoiseParams()

    def call():
        ctx.set_option("denoise_tiling", tiling)
        if route is None:
            R.denoise(hist[1], feat[1], out, params)
        else:
            ctx.set_option("variance_prefilter", route)
            R.denoise_variance(hist[1], feat[1], mom[1], out, params)
    return call


SETS = [("reproject, staging %d" % g, reproject_call(False, g)) for g in (0, 1)] + [("reproject_moments, staging %d" % g, reproject_call(True, g)) for g in (0, 1)] \
    + [("denoise, rule", filter_call(-1, None))] + [("variance, rule, g route %d" % r, filter_call(-1, r)) for r in (0, 1)] \
    + [("estimate + 1 level, %s short" % n, filter_call(-1, 0, levels=1, min_history=m)) for n, m in (("all", 64), ("none", 1))] \
    + [("variance, tiling %d, g route %d" % (t, r), filter_call(t, r)) for t in (0, 1) for r in (0, 1)]
for frames in (2, 6):
    fill(frames)
    res = {name: [] for name, _ in SETS}
    for rnd in range(2):              # the sets interleaved, twice: drift of the box's clock shows as a difference between the rounds
        for name, call in SETS:
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
    n_hist = hist[1].read_float().reshape(-1, 4)[:, 3]
    print("%s %dx%d %d spp, %d frames: history length median %d, %.1f %% of the pixels below 4" % (cfg, W, H, spp, frames, np.median(n_hist), 100.0 * ((n_hist > 0) & (n_hist < 4)).mean()))
    for name, _ in SETS:
        a = np.array(res[name])
        print("  %-34s median %.4f  min %.4f  (rounds %.4f / %.4f) ms per call" % (name, np.median(a), a.min(), np.median(a[:12]), np.median(a[12:])))
ctx.set_option("denoise_tiling", -1), ctx.set_option("variance_prefilter", -1), ctx.set_option("reproject_staging", -1)
