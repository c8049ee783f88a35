#!/usr/bin/env python3
"""tools/feature_bench.py CONFIG [K ...]  -- ON THE GPU BOX: what a feature call (rtw_render_features) costs beside the nearest thing the
renderer itself offers, a preview render (use_base_color) of the same passes, in the style of tools/ab.py: per set 3 warm-up calls and 12 timed
calls of K passes, the sets interleaved twice.  Timed with HIP events on the context's stream (torch's: the context is made from it), so the
figure is the time the launches take on the device, without the host's call overhead.  Prints median / min ms per CALL of each set.
CONFIG as bench.CONFIGS (c2, c4, setup = the default scene ...); K defaults to 1 and 20."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import raytracerwin_amd as R  # noqa: E402
import bench  # noqa: E402

cfg = sys.argv[1]
KS = [int(v) for v in sys.argv[2:]] or [1, 20]
mesh, W, H, spp, depth, kind = bench.CONFIGS[cfg]
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
feat = R.FeatureBuffers(ctx, W, H)
preview = R.RenderOption(True)
SETS = [("features", lambda p, k: s.render_features(feat, 10, 0, 1, p, k, spp, 12345)),
        ("preview render", lambda p, k: s.render_passes(fb, 10, 0, 1, depth, preview, p, k, spp, 12345))]
print("%s %dx%d %d spp" % (cfg, W, H, spp))
for K in KS:
    res = {name: [] for name, _ in SETS}
    for rnd in range(2):          # the sets interleaved, twice: drift of the box's clock shows as a difference between the rounds
        for name, call in SETS:
            p = 0
            for i in range(3):
                call(p, K); p += K
            ctx.synchronize()
            for i in range(12):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                call(p, K); p += K
                t1.record()
                t1.synchronize()
                res[name].append(t0.elapsed_time(t1))
    base = np.median(np.array(res["preview render"]))
    for name, _ in SETS:
        a = np.array(res[name])
        print("  K=%-3d %-16s median %.4f  min %.4f  (rounds %.4f / %.4f) ms per call   x %.2f of the preview render" %
              (K, name, np.median(a), a.min(), np.median(a[:12]), np.median(a[12:]), np.median(a) / base))
