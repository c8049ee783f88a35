#!/usr/bin/env python3
"""tools/tonemap_bench.py [--sizes 1920x1080,3840x2160] [--repeats 9] [--inner 20]
ON THE GPU BOX: same-session A/B of rtw_tonemap.  In ONE process, interleaved as tools/ab.py does, it times -- HIP events around `inner` back-to-back
calls, after a warm-up, an odd number of times each; the figure is milliseconds per call --
  linear / reinhard / aces      tonemap with an Exposure (metering on), the default "tonemap_histogram", on a rendered frame of the setup scene
  hold                          ACES under HOLD: the same traffic without the histogram
  h0_frame / h1_frame           ACES, "tonemap_histogram" 0 (an LDS atomic per lane) and 1 (wave-aggregated), the rendered frame
  h0_flat / h1_flat             the same on a flat grey frame: every pixel in one bin, the contention worst case
  meter                         meter_exposure alone (16 bytes per pixel in, nothing out)
  atrous1 / atrous2             denoise with 1 and with 2 levels on the same frame: their difference is one a-trous level, a kernel of similar traffic
  torch                         the route a caller takes without the call, on the same wrapped tensors: divide, luminance, histc over the same bins, the
                                percentile-window mean and exposure (on the device, no read-back), ACES, gamma by pow, pack
and prints median / min / max per variant as one JSON line per size.  The two histogram settings are compared bit for bit first."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import raytracerwin_amd as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="1920x1080,3840x2160")
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--inner", type=int, default=20)
args = ap.parse_args()
assert args.repeats % 2 == 1, "an odd number of repeats (the median is then a measured value)"

import torch  # noqa: E402
if not torch.cuda.is_available():
    raise SystemExit("tonemap_bench: no GPU -- nothing is measured on the CPU")
from raytracerwin_amd.setup_scene import SetupScene  # noqa: E402

ctx = R.Context(0, stream=torch.cuda.current_stream().cuda_stream)
s = R.RayTracerScene(ctx)
SetupScene(s, os.path.join(ROOT, "assets", "unitychan.obj"))
s.commit()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / args.inner


for size in args.sizes.split(","):
    W, H = [int(v) for v in size.split("x")]
    n = W * H
    acc_t = torch.zeros((n, 4), dtype=torch.float32, device="cuda"); argb_t = torch.zeros((n,), dtype=torch.int32, device="cuda")
    flat_t = torch.full((n, 4), 0.5, dtype=torch.float32, device="cuda"); flat_t[:, 3] = torch.tensor(1, dtype=torch.int32).view(torch.float32)
    out_t = torch.empty_like(acc_t); out_argb_t = torch.empty_like(argb_t)
    frame, flat = R.Framebuffer(ctx, W, H, acc_t.data_ptr(), argb_t.data_ptr()), R.Framebuffer(ctx, W, H, flat_t.data_ptr(), argb_t.data_ptr())
    dst = R.Framebuffer(ctx, W, H, out_t.data_ptr(), out_argb_t.data_ptr())
    feats, e = R.FeatureBuffers(ctx, W, H), R.Exposure(ctx)
    s.render_passes(frame, 10, 0, 1, 4, None, 0, 2, 4, 12345)
    s.render_features(feats, 10, 0, 1, 0, 1, 1, 12345)
    P = {k: R.TonemapParams(curve=c) for k, c in (("linear", 0), ("reinhard", 1), ("aces", 2))}
    hold = R.TonemapParams(flags=R.TonemapParams.HOLD)

    def call(src, p, hist=-1, ex=e):
        ctx.set_option("tonemap_histogram", hist)
        R.tonemap(src, dst, ex, p)

    def torch_route():
        c = acc_t[:, :3] / acc_t[:, 3:4].view(torch.int32).float()
        L = 0.2126 * c[:, 0] + 0.7152 * c[:, 1] + 0.0722 * c[:, 2]
        bins = ((L.view(torch.int32) >> 20) - 856).clamp(0, 255).float()
        h = torch.histc(torch.where((L > 0) & torch.isfinite(L), bins, torch.full_like(bins, -1.0)), bins=256, min=0, max=256)
        Pk = torch.cumsum(h, 0) - h
        N = h.sum()
        ck = (torch.minimum(Pk + h, 0.95 * N) - torch.maximum(Pk, 0.5 * N)).clamp_min(0)
        m = (ck * torch.arange(256, device="cuda")).sum() / ck.sum().clamp_min(1)
        E = (0.18 / torch.exp2((m + 0.5) / 8 - 20)).clamp(1 / 64, 64)
        v = (c * E).clamp_min(0)
        y = (v * (2.51 * v + 0.03)) / (v * (2.43 * v + 0.59) + 0.14)
        k = (y.clamp(0, 1).pow(1 / 2.2) * 255).to(torch.int32)
        out_t[:, :3] = y
        out_argb_t.copy_((255 << 24) - (1 << 32) + (k[:, 0] << 16) + (k[:, 1] << 8) + k[:, 2])

    variants = {"linear": lambda: call(frame, P["linear"]), "reinhard": lambda: call(frame, P["reinhard"]), "aces": lambda: call(frame, P["aces"]),
                "hold": lambda: call(frame, hold), "h0_frame": lambda: call(frame, P["aces"], 0), "h1_frame": lambda: call(frame, P["aces"], 1),
                "h0_flat": lambda: call(flat, P["aces"], 0), "h1_flat": lambda: call(flat, P["aces"], 1), "meter": lambda: R.meter_exposure(frame, e, P["aces"]),
                "atrous1": lambda: R.denoise(frame, feats, dst, R.DenoiseParams(levels=1)), "atrous2": lambda: R.denoise(frame, feats, dst, R.DenoiseParams(levels=2)),
                "torch": torch_route}
    got = []
    for hist in (0, 1):         # the same bits either way: one metered call each from a fresh object
        e.reset(); call(frame, P["aces"], hist)
        got.append((e.read(), out_t.cpu().numpy().view(np.uint32), out_argb_t.cpu().numpy()))
    assert got[0][0][0] == got[1][0][0] and (got[0][0][2] == got[1][0][2]).all() and (got[0][1] == got[1][1]).all() and (got[0][2] == got[1][2]).all(), "the two histograms differ"
    for f in variants.values():       # warm-up
        f(); f()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(args.repeats):      # interleaved: drift of the box shows in every variant alike
        for k, f in variants.items():
            ms[k].append(timed(f))
    ctx.set_option("tonemap_histogram", -1)
    res = {"tool": "tonemap_bench", "size": size, "metered_pixels": int(got[0][0][2].sum()), "bins_used": int((got[0][0][2] > 0).sum()), "repeats": args.repeats,
           "inner": args.inner, "device": torch.cuda.get_device_name(0), "library": R.library().rtw_version().decode()}
    for k, v in ms.items():
        v = sorted(v)
        res[k] = {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}
    print(json.dumps(res), flush=True)
    for o in (e, feats, dst, flat, frame):
        o.close()
s.close(); ctx.close()
