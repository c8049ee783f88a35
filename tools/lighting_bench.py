#!/usr/bin/env python3
"""tools/lighting_bench.py --scene TorusKnot|setup [--configs 1x1,4x4] [--repeats 7]
ON THE GPU BOX: same-session A/B of rtw_render_lighting at 1920x1080.  In ONE process, interleaved as tools/ab.py does, it times -- HIP events
around one call, after a warm-up, an odd number of times each --
  deal0 / deal1     render_lighting, one pass, "lighting_deal" 0 (positional) and 1 (compacted); their frames are compared bit for bit first
  route             the route without the call, on the same features: the shadow rays of every (light, sample, casting pixel) built by a torch
                    expression (a culled job becomes a ray of length 0), trace_occluded, a torch reduction
  query             trace_occluded alone on the route's ray array (the same ray count)
and prints median / min / max per variant as one JSON line per configuration LIGHTS x SAMPLES.  1x1 is one point light without a radius; with more
lights they have radii, and the route moves them by unit vectors of the table's distribution drawn outside the timed region (the timing is what
matters).  Without radii the route's per-pixel values are compared with the call's: the share of casting pixels that differ by more than 1e-3 (the
route rounds its origins differently, so pixels on a shadow's edge may fall on its other side)."""
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
ap.add_argument("--configs", default="1x1,4x4")
ap.add_argument("--repeats", type=int, default=7)
args = ap.parse_args()
assert args.repeats % 2 == 1, "an odd number of repeats (the median is then a measured value)"

import torch  # noqa: E402
if not torch.cuda.is_available():
    raise SystemExit("lighting_bench: no GPU -- nothing is measured on the CPU")

W, H, SEED = 1920, 1080, 12345
# (type, v, radius): the reference's own light first
LIGHTS = [(0, (0.0, -4.5, 0.0), 0.3), (0, (3.0, 4.0, 5.0), 0.3), (1, (0.0, 0.8, 0.6), 0.05), (0, (-4.0, 2.0, 3.0), 0.3)]
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
cast = np.flatnonzero((albedo[:, 3] > 0) & (ids[:, 0] >= 0))
cam = s.get_camera()
rays0 = np.ascontiguousarray(R.camera_rays(cam, W, H, cast.astype(np.int32), 0, 0, SEED), np.float32)
n_d = torch.from_numpy(geom[cast, 0:3] / albedo[cast, 3:4]).cuda()
n_d = n_d / n_d.norm(dim=1, keepdim=True)
P_d = torch.from_numpy(rays0[:, 0:3] + rays0[:, 3:6] * (geom[cast, 3:4] / albedo[cast, 3:4])).cuda()
N = len(cast)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


for NL, S in [tuple(int(v) for v in c.split("x")) for c in args.configs.split(",")]:
    soft = NL > 1
    lights = [R.Light(t, 0, v, (1.0, 1.0, 1.0), r if soft else 0.0) for t, v, r in LIGHTS[:NL]]
    p = R.LightingParams(samples=S, flags=0)
    O_d = P_d + n_d * p.bias
    u_d = torch.nn.functional.normalize(torch.randn((NL, S, N, 3), device="cuda"), dim=3) if soft else torch.zeros((NL, S, N, 3), device="cuda")
    v_d = torch.tensor([l.v[:] for l in lights], device="cuda").view(NL, 1, 1, 3)
    r_d = torch.tensor([l.radius for l in lights], device="cuda").view(NL, 1, 1, 1)
    point = torch.tensor([l.type == 0 for l in lights], device="cuda").view(NL, 1, 1)
    rays = torch.empty((NL * S * N, 7), dtype=torch.float32, device="cuda")
    occ = torch.empty((NL * S * N,), dtype=torch.uint8, device="cuda")
    out = torch.empty((N,), dtype=torch.float32, device="cuda")

    def build():
        D = v_d + u_d * r_d
        D = torch.where(point.unsqueeze(3), D - O_d, D)
        ln = D.norm(dim=3)
        d = D / ln.unsqueeze(3)
        c = (d * n_d).sum(dim=3)
        live = c > 0
        r = rays.view(NL, S, N, 7)
        r[..., 0:3] = O_d
        r[..., 3:6] = d
        r[..., 6] = torch.where(live, torch.where(point, ln, torch.full_like(ln, 1000.0)), torch.zeros_like(ln))
        return c, live

    def route():
        c, live = build()
        s.trace_occluded(rays, out=occ)
        t = torch.where((occ.view(NL, S, N) != 0) | ~live, torch.zeros_like(c), c)
        out.copy_((t.sum(dim=1) / S).sum(dim=0))

    def call(deal):
        ctx.set_option("lighting_deal", deal)
        s.render_lighting(fb, dst, lights, p, 0, 1, SEED)

    variants = {"deal0": lambda: call(0), "deal1": lambda: call(1), "route": route, "query": lambda: s.trace_occluded(rays, out=occ)}
    dst.clear(); call(0); a0 = dst.read_float(); g0 = dst.resolve_argb(); dst.clear(); call(1); a1 = dst.read_float(); g1 = dst.resolve_argb()
    assert (a0.view(np.uint32) == a1.view(np.uint32)).all() and (g0 == g1).all(), "the two deals differ"
    c, live = build(); route(); torch.cuda.synchronize()
    # (a pixel on a shadow's edge can fall on either side of it: the route's origins are rounded differently)
    diff = None if soft else float((np.abs(a0[cast, 0] - out.cpu().numpy()) > 1e-3).mean())
    for f in variants.values():       # warm-up
        f(); f()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(args.repeats):      # interleaved: drift of the box shows in every variant alike
        for k, f in variants.items():
            ms[k].append(timed(f))
    ctx.set_option("lighting_deal", -1)
    res = {"tool": "lighting_bench", "scene": args.scene, "lights": NL, "samples": S, "casting_pixels": int(N), "jobs": int(NL * S * N),
           "live_jobs": int(live.sum().item()), "route_share_of_pixels_off_by_1e-3": diff, "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
           "library": R.library().rtw_version().decode()}
    for k, v in ms.items():
        v = sorted(v)
        res[k] = {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}
    print(json.dumps(res), flush=True)
dst.close(); fb.close(); s.close(); ctx.close()
