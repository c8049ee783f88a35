#!/usr/bin/env python3
"""tools/denoise_bench.py CONFIG [WxH]  -- ON THE GPU BOX: what rtw_denoise costs on a one-pass frame of CONFIG (bench.CONFIGS; WxH overrides its frame
size), in the style of tools/feature_bench.py: HIP events on the context's stream around each call, per set 3 warm-up and 12 timed calls, the sets
interleaved twice.  The sets: "denoise_tiling" 0 (dense), 1 (lattice) and -1 (the rule) at 1 .. 5 levels with the default sigmas and flags, and beside
them the one-pass rtw_render_passes + rtw_render_features that fill the buffers.  A level's own cost is printed as the difference between the medians
at k and k - 1 levels (the level of step 2^(k-1); the last level's extra work -- remodulation, pack, 20 instead of 16 bytes out -- stays in every figure).
The floor is the traffic of one call at 8 TB/s: prepare 56 B in + 36 B out, a level 36 B in + 16 B out, the last level 36 + 16 B in and 20 B out."""
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
fb, out, feat = R.Framebuffer(ctx, W, H), R.Framebuffer(ctx, W, H), R.FeatureBuffers(ctx, W, H)


def fill():
    fb.clear(); feat.clear()
    s.render_passes(fb, 10, 0, 1, depth, None, 0, 1, spp, 12345)
    s.render_features(feat, 10, 0, 1, 0, 1, spp, 12345)


def filter_call(tiling, levels):
    params = R.DenoiseParams(levels=levels)

    def call():
        ctx.set_option("denoise_tiling", tiling)
        R.denoise(fb, feat, out, params)
    return call


LEVELS = range(1, 6)
SETS = [("render + features", fill)] + [("tiling %2d, %d levels" % (t, k), filter_call(t, k)) for t in (0, 1, -1) for k in LEVELS]
fill()
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
    fill()
ctx.set_option("denoise_tiling", -1)
n = W * H
print("%s %dx%d %d spp; traffic floor at 8 TB/s: %.4f ms for 5 levels, %.4f ms per further level" % (cfg, W, H, spp, n * (92 + 4 * 52 + 72) / 8e9, n * 52 / 8e9))
med = {}
for name, _ in SETS:
    a = np.array(res[name])
    med[name] = np.median(a)
    print("  %-22s median %.4f  min %.4f  (rounds %.4f / %.4f) ms per call" % (name, med[name], a.min(), np.median(a[:12]), np.median(a[12:])))
for t in (0, 1, -1):
    m = [med["tiling %2d, %d levels" % (t, k)] for k in LEVELS]
    print("  tiling %2d per level: step 1 + prepare %.4f" % (t, m[0]) + "".join("  step %d %.4f" % (1 << k, m[k] - m[k - 1]) for k in range(1, len(m))))
