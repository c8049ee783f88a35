#!/usr/bin/env python3
"""tools/reproject_bench.py [CONFIG]  -- ON THE GPU BOX: what rtw_reproject costs on one-pass frames of CONFIG (bench.CONFIGS, default c2) at 1920x1080 and
3840x2160, in the style of tools/denoise_bench.py: HIP events on the context's stream around each call, per set 3 warm-up and 12 timed calls, the sets
interleaved twice.  The sets: "reproject_staging" 0 (direct), 1 (staged) and -1 (the rule) for four motions of the previous camera -- none, a pan, a
dolly, and a 40 degree roll about the view axis, which defeats staging -- and beside them ONE level of rtw_denoise on the same frame (the yardstick of
a kernel that moves as many records).  The floor is the traffic of a call at 8 TB/s: 56 B current inputs + 56 B history + 20 B written per pixel."""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import raytracerwin_amd as R  # noqa: E402
import bench  # noqa: E402

cfg = sys.argv[1] if len(sys.argv) > 1 else "c2"
mesh, _, _, spp, depth, kind = bench.CONFIGS[cfg]
torch.cuda.init()
ctx = R.Context(0, stream=torch.cuda.current_stream().cuda_stream)
s = R.RayTracerScene(ctx)
if kind == "setup":
    from raytracerwin_amd.setup_scene import SetupScene
    SetupScene(s, os.path.join(ROOT, "assets", mesh + ".obj"))
else:
    s.AddShape(R.RMeshShape.Create(os.path.join(ROOT, "assets", mesh + ".obj")), bench.make_material(R, kind))
s.commit()
EYE = (0.0, 0.0, 7.0)
rolled = (math.sin(math.radians(40.0)), math.cos(math.radians(40.0)), 0.0)
MOTIONS = [("none", R.Camera.look_at(EYE, (0, 0, 0))), ("pan", R.Camera.look_at((0.3, 0.0, 7.0), (0.3, 0, 0))),
           ("dolly", R.Camera.look_at((0.0, 0.0, 7.7), (0, 0, 0))), ("roll 40", R.Camera.look_at(EYE, (0, 0, 0), up=rolled))]
cur_cam = MOTIONS[0][1]

for W, H in ((1920, 1080), (3840, 2160)):
    cur, out, f_cur = R.Framebuffer(ctx, W, H), R.Framebuffer(ctx, W, H), R.FeatureBuffers(ctx, W, H)
    hist = {}
    for k, (name, cam) in enumerate([("current", cur_cam)] + MOTIONS):       # the history of each motion: a frame rendered from its camera
        fb, feat = (cur, f_cur) if k == 0 else (R.Framebuffer(ctx, W, H), R.FeatureBuffers(ctx, W, H))
        fb.clear(); feat.clear()
        s.set_camera(cam)
        s.render_passes(fb, 10, 0, 1, depth, None, 0, 1, spp, 12345 + k)
        s.render_features(feat, 10, 0, 1, 0, 1, spp, 12345 + k)
        hist[name] = (fb, feat, cam)

    def reproject_call(staging, name):
        fb, feat, cam = hist[name]

        def call():
            ctx.set_option("reproject_staging", staging)
            R.reproject(cur_cam, cam, cur, f_cur, fb, feat, out)
        return call

    def level_call(levels):
        params = R.DenoiseParams(levels=levels)
        return lambda: R.denoise(cur, f_cur, out, params)

    SETS = [("denoise, %d level%s" % (k, "s" * (k > 1)), level_call(k)) for k in (1, 2)] \
        + [("staging %2d, %s" % (st, name), reproject_call(st, name)) for name, _ in MOTIONS for st in (0, 1, -1)]
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
    ctx.set_option("reproject_staging", -1)
    print("%s %dx%d %d spp; traffic floor at 8 TB/s: %.4f ms" % (cfg, W, H, spp, W * H * 132 / 8e9))
    for name, _ in SETS:
        a = np.array(res[name])
        print("  %-22s median %.4f  min %.4f  (rounds %.4f / %.4f) ms per call" % (name, np.median(a), a.min(), np.median(a[:12]), np.median(a[12:])))
    print("  one a-trous level (step 2, not the last): %.4f ms" % (np.median(res["denoise, 2 levels"]) - np.median(res["denoise, 1 level"])))
    for fb, feat, _ in hist.values():
        fb.close(); feat.close()
    out.close()
