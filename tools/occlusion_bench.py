#!/usr/bin/env python3
"""tools/occlusion_bench.py --scene TorusKnot|setup [--samples 4,16] [--radius 0.25,1000] [--repeats 7]
ON THE GPU BOX: same-session A/B of rtw_render_occlusion at 1920x1080.  In ONE process, interleaved as tools/ab.py does, it times -- HIP events
around one call, after a warm-up, an odd number of times each --
  order0 / order1   render_occlusion, one pass, "occlusion_order" 0 (a lane per pixel) and 1 (a lane per sample)
  route             today's three-kernel route on the same features: the rays built by a torch expression (origin, hemisphere direction from the same
                    unit-table entries, gathered from a device copy of the indices made outside the timed region), trace_occluded, a torch reduction
  query             trace_occluded alone on the route's ray array (the same ray count)
and prints median / min / max per variant as one JSON line per (samples, radius).  The route's per-pixel values are compared with the call's first
(equal up to the order of a float sum: the route reduces with torch.sum)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import raytracerwin_amd as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scene", default="TorusKnot", choices=["TorusKnot", "setup"])
ap.add_argument("--samples", default="4,16")
ap.add_argument("--radius", default="0.25,1000")
ap.add_argument("--repeats", type=int, default=7)
args = ap.parse_args()
assert args.repeats % 2 == 1, "an odd number of repeats (the median is then a measured value)"

import torch  # noqa: E402
if not torch.cuda.is_available():
    raise SystemExit("occlusion_bench: no GPU -- nothing is measured on the CPU")
from camera_support import rand31  # noqa: E402  (the stream's hash, vectorised)

W, H, SEED = 1920, 1080, 12345
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
# the route's inputs on the device: mean normal, first-hit point (camera ray x depth), and per (sample, casting pixel) the unit-table entry
cam = s.get_camera()
rays0 = np.ascontiguousarray(R.camera_rays(cam, W, H, cast.astype(np.int32), 0, 0, SEED), np.float32)
n_d = torch.from_numpy(geom[cast, 0:3] / albedo[cast, 3:4]).cuda()
n_d = n_d / n_d.norm(dim=1, keepdim=True)
P_d = torch.from_numpy(rays0[:, 0:3] + rays0[:, 3:6] * (geom[cast, 3:4] / albedo[cast, 3:4])).cuda()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


for S in [int(v) for v in args.samples.split(",")]:
    idx = np.stack([rand31(SEED, cast, (0 * 64 + k) | 0x40000000, 0).astype(np.int64) % 0xFFFFFF for k in range(S)])
    uniq, inv = np.unique(idx, return_inverse=True)
    table = np.stack([R.api.unit_table_entry(int(i)) for i in uniq]) if len(uniq) <= 200000 else None
    if table is None:       # too many entries for the one-at-a-time host call: directions of the same distribution instead (the timing is what matters)
        r = np.random.default_rng(1).standard_normal((len(uniq), 3)).astype(np.float32)
        table = r / np.linalg.norm(r, axis=1, keepdims=True)
    v_d = torch.from_numpy(table[inv.reshape(idx.shape)]).cuda()           # (S, n, 3)
    for radius in [float(v) for v in args.radius.split(",")]:
        p = R.OcclusionParams(radius=radius, samples=S)
        rays = torch.empty((S * len(cast), 7), dtype=torch.float32, device="cuda")
        occ = torch.empty((S * len(cast),), dtype=torch.uint8, device="cuda")
        out = torch.empty((len(cast),), dtype=torch.float32, device="cuda")

        def build():
            dt = (v_d * n_d).sum(dim=2, keepdim=True)
            d = torch.where(dt > 0, v_d, v_d - (n_d * 2.0) * dt)
            r = rays.view(S, -1, 7)
            r[:, :, 0:3] = P_d + n_d * p.bias
            r[:, :, 3:6] = d
            r[:, :, 6] = radius
            return d

        def route():
            d = build()
            s.trace_occluded(rays, out=occ)
            c = (d * n_d).sum(dim=2).clamp_min(0.0)
            t = torch.where(occ.view(S, -1) != 0, torch.zeros_like(c), c)
            wt = c.sum(dim=0)
            out.copy_(torch.where(wt > 0, t.sum(dim=0) / wt, torch.ones_like(wt)))

        def call(order):
            ctx.set_option("occlusion_order", order)
            s.render_occlusion(fb, dst, p, 0, 1, SEED)

        variants = {"order0": lambda: call(0), "order1": lambda: call(1), "route": route, "query": lambda: s.trace_occluded(rays, out=occ)}
        dst.clear(); call(0); a0 = dst.read_float(); dst.clear(); call(1); a1 = dst.read_float(); route(); torch.cuda.synchronize()
        assert (a0.view(np.uint32) == a1.view(np.uint32)).all(), "the two orders differ"
        diff = float(np.abs(a0[cast, 0] - out.cpu().numpy()).max()) if table is not None and len(uniq) <= 200000 else None
        for f in variants.values():       # warm-up
            f(); f()
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(args.repeats):      # interleaved: drift of the box shows in every variant alike
            for k, f in variants.items():
                ms[k].append(timed(f))
        ctx.set_option("occlusion_order", -1)
        res = {"tool": "occlusion_bench", "scene": args.scene, "samples": S, "radius": radius, "casting_pixels": int(len(cast)), "rays": int(S * len(cast)),
               "route_max_abs_difference": diff, "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "library": R.library().rtw_version().decode()}
        for k, v in ms.items():
            v = sorted(v)
            res[k] = {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}
        print(json.dumps(res), flush=True)
dst.close(); fb.close(); s.close(); ctx.close()
