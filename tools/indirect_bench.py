#!/usr/bin/env python3
"""tools/indirect_bench.py --scene TorusKnot|setup [--configs 1x1,4x2,8x8] [--repeats 7]
ON THE GPU BOX: same-session A/B of rtw_render_indirect at 1920x1080.  In ONE process, interleaved as tools/ab.py does, it times -- HIP events
around one call, after a warm-up, an odd number of times each --
  deal0 / deal1     render_indirect, one pass, "indirect_deal" 0 (positional) and 1 (compacted); their frames are compared bit for bit first
  unstaged          the rule's deal (-1) with "indirect_staging" 0: 256-thread blocks, nothing in LDS but the block's own words (deal0 / deal1 run with 1)
  occlusion         render_occlusion with the configuration's samples, radius 1000: the gather rays as any-hit walks
  lighting          render_lighting with the configuration's lights x samples: a superset of the gather hits' shadow rays
and prints median / min / max per variant as one JSON line per configuration SAMPLES x LIGHTS; `sum` is occlusion + lighting of the same repeat."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import raytracerwin_amd as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scene", default="TorusKnot", choices=["TorusKnot", "setup"])
ap.add_argument("--configs", default="1x1,4x2,8x8")
ap.add_argument("--repeats", type=int, default=7)
args = ap.parse_args()
assert args.repeats % 2 == 1, "an odd number of repeats (the median is then a measured value)"

import torch  # noqa: E402
if not torch.cuda.is_available():
    raise SystemExit("indirect_bench: no GPU -- nothing is measured on the CPU")

W, H, SEED = 1920, 1080, 12345
# (type, v, radius): the reference's own light first
LIGHTS = [(0, (0.0, -4.5, 0.0), 0.3), (0, (3.0, 4.0, 5.0), 0.3), (1, (0.0, 0.8, 0.6), 0.05), (0, (-4.0, 2.0, 3.0), 0.3),
          (0, (5.0, 1.0, -2.0), 0.3), (1, (0.6, 0.8, 0.0), 0.05), (0, (-2.0, 5.0, -4.0), 0.3), (0, (0.0, 6.0, 0.0), 0.3)]
ctx = R.Context(0, stream=torch.cuda.current_stream().cuda_stream)
s = R.RayTracerScene(ctx)
if args.scene == "setup":
    from raytracerwin_amd.setup_scene import SetupScene
    SetupScene(s, os.path.join(ROOT, "assets", "unitychan.obj"))
else:
    s.AddShape(R.RMeshShape.Create(os.path.join(ROOT, "assets", "TorusKnot.obj")), R.SurfaceMaterial_Diffuse())
s.commit()
fb, dst = R.FeatureBuffers(ctx, W, H), R.Framebuffer(ctx, W, H)
s.render_features(fb, 10, 0, 1, 0, 1, 1, SEED)
geom, albedo, ids = fb.read()
casting = int(((albedo[:, 3] > 0) & (ids[:, 0] >= 0)).sum())


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


for S, NL in [tuple(int(v) for v in c.split("x")) for c in args.configs.split(",")]:
    lights = [R.Light(t, 0, v, (1.0, 1.0, 1.0), r if NL > 1 else 0.0) for t, v, r in LIGHTS[:NL]]
    pi, po, pl = R.IndirectParams(samples=S, flags=0), R.OcclusionParams(samples=S, radius=1000.0), R.LightingParams(samples=S, flags=0)

    def call(deal, staging=1):
        ctx.set_option("indirect_deal", deal)
        ctx.set_option("indirect_staging", staging)
        s.render_indirect(fb, dst, lights, pi, 0, 1, SEED)

    variants = {"deal0": lambda: call(0), "deal1": lambda: call(1), "unstaged": lambda: call(-1, 0), "occlusion": lambda: s.render_occlusion(fb, dst, po, 0, 1, SEED),
                "lighting": lambda: s.render_lighting(fb, dst, lights, pl, 0, 1, SEED)}
    dst.clear(); call(0); a0 = dst.read_float(); g0 = dst.resolve_argb(); dst.clear(); call(1); a1 = dst.read_float(); g1 = dst.resolve_argb()
    assert (a0.view(np.uint32) == a1.view(np.uint32)).all() and (g0 == g1).all(), "the two deals differ"
    for f in variants.values():       # warm-up
        f(); f()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(args.repeats):      # interleaved: drift of the box shows in every variant alike
        for k, f in variants.items():
            ms[k].append(timed(f))
    call(-1, -1)
    ms["sum"] = [a + b for a, b in zip(ms["occlusion"], ms["lighting"])]
    res = {"tool": "indirect_bench", "scene": args.scene, "samples": S, "lights": NL, "casting_pixels": casting, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0), "library": R.library().rtw_version().decode()}
    for k, v in ms.items():
        v = sorted(v)
        res[k] = {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}
    print(json.dumps(res), flush=True)
dst.close(); fb.close(); s.close(); ctx.close()
