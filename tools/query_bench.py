#!/usr/bin/env python3
"""tools/query_bench.py --mesh TorusKnot|BlenderMonkey|unitychan|setup [--rays N] [--kind camera|bounce|shadow[,...]] [--repeats 7]
ON THE GPU BOX: same-session A/B of the device-buffer ray queries.  In ONE process, interleaved as tools/ab.py does, it times
"query_kernel" 0 (closest_kernel on the caller's buffers: the parent's own kernel, the baseline) and 1 (qtrace_kernel) for the closest-hit and the
any-hit query -- HIP events around one call, after a warm-up (which also grows the baseline's stand-in buffer outside the timed region) --
an odd number of times each, and prints median / min / max per variant as one JSON line per ray kind.
The host entry rtw_trace_closest (copies + wait) is timed end to end, for context.

  camera  camera_rays of a 1920x1080 frame (the first N pixels of an even spread over the frame)
  bounce  from the camera rays' hit points, seeded cosine-ish directions (normal + unit vector), distance 1000
  shadow  from the hit points towards a fixed light, as long as the way there
All inputs are generated on the host once and uploaded once.  The two kernels' outputs are compared before anything is timed."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import raytracerwin_amd as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--mesh", default="TorusKnot", choices=["TorusKnot", "BlenderMonkey", "unitychan", "setup"])
ap.add_argument("--rays", type=int, default=1920 * 1080)
ap.add_argument("--kind", default="camera")
ap.add_argument("--repeats", type=int, default=7)
args = ap.parse_args()
assert args.repeats % 2 == 1, "an odd number of repeats (the median is then a measured value)"

import torch  # noqa: E402
if not torch.cuda.is_available():
    raise SystemExit("query_bench: no GPU -- nothing is measured on the CPU")

ctx = R.Context(0, stream=torch.cuda.current_stream().cuda_stream)
s = R.RayTracerScene(ctx)
if args.mesh == "setup":
    from raytracerwin_amd.setup_scene import SetupScene
    SetupScene(s, os.path.join(ROOT, "assets", "unitychan.obj"))
else:
    s.AddShape(R.RMeshShape.Create(os.path.join(ROOT, "assets", args.mesh + ".obj")), R.SurfaceMaterial_Diffuse())
s.commit()

W, H = 1920, 1080
n = min(args.rays, W * H)
pixels = np.linspace(0, W * H - 1, n).astype(np.int32)
camera = np.ascontiguousarray(R.camera_rays(s.get_camera(), W, H, pixels, 0, 0, 12345), np.float32)


def secondary(kind):
    hits, shape, _ = s.FindIntersectionWithScene(camera)
    h = hits[shape >= 0]
    o = h[:, 0:3] + h[:, 3:6] * np.float32(1e-3)
    if kind == "shadow":
        d = np.array([4.0, 6.0, 5.0], np.float32) - o
        ln = np.sqrt((d * d).sum(axis=1, dtype=np.float32))
    else:
        rng = np.random.default_rng(20261020)
        u = rng.standard_normal((len(o), 3)).astype(np.float32)
        d = h[:, 3:6] + u / np.linalg.norm(u, axis=1, keepdims=True)
        ln = np.full(len(o), 1000.0, np.float32)
    d = d / np.maximum(np.linalg.norm(d, axis=1, keepdims=True), np.float32(1e-20))
    rays = np.concatenate([o, d, ln[:, None]], axis=1).astype(np.float32)
    reps = -(-n // max(1, len(rays)))       # as many rays as the camera set
    return np.ascontiguousarray(np.tile(rays, (reps, 1))[:n])


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def options(**kv):
    ctx.set_option("query_kernel", kv.get("query_kernel", -1))


for kind in args.kind.split(","):
    host = camera if kind == "camera" else secondary(kind)
    rays = torch.from_numpy(host).cuda()
    hits = torch.empty((n, 11), dtype=torch.float32, device="cuda")
    shape = torch.empty((n,), dtype=torch.int32, device="cuda")
    tri = torch.empty((n,), dtype=torch.int32, device="cuda")
    occ = torch.empty((n,), dtype=torch.uint8, device="cuda")
    variants = {"closest_k0": (dict(query_kernel=0), False), "closest_k1": (dict(query_kernel=1), False),
                "any_k0": (dict(query_kernel=0), True), "any_k1": (dict(query_kernel=1), True)}

    def call(name):
        opts, any_hit = variants[name]
        options(**opts)
        if any_hit:
            s.trace_occluded(rays, out=occ)
        else:
            s.trace_closest(rays, hits=hits, shape=shape, tri=tri)

    # faster and different is not faster: the outputs first
    ref = {}
    for name in variants:
        call(name)
        torch.cuda.synchronize()
        got = (occ.clone(),) if variants[name][1] else (hits.clone(), shape.clone(), tri.clone())
        key = "any" if variants[name][1] else "closest"
        if key in ref:
            assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(got, ref[key])), name + " differs from the baseline"
        else:
            ref[key] = got
    for name in variants:       # warm-up
        for _ in range(2):
            call(name)
    torch.cuda.synchronize()
    ms = {name: [] for name in variants}
    for _ in range(args.repeats):      # interleaved: drift of the box shows in every variant alike
        for name in variants:
            ms[name].append(timed(lambda: call(name)))
    options()
    t0 = time.perf_counter()
    s.FindIntersectionWithScene(host)
    host_ms = (time.perf_counter() - t0) * 1e3
    out = {"tool": "query_bench", "mesh": args.mesh, "kind": kind, "rays": n, "hit_fraction": round(float((ref["any"][0] != 0).float().mean().item()), 4), "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0), "library": R.library().rtw_version().decode(), "host_entry_rtw_trace_closest_ms": round(host_ms, 3)}
    for name, v in ms.items():
        v = sorted(v)
        out[name] = {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}
    for q in ("closest", "any"):
        b, k = out[q + "_k0"], out[q + "_k1"]
        out[q + "_bar_met"] = bool(b["median_ms"] - k["median_ms"] > b["max_ms"] - b["min_ms"])
    out["any_not_slower_than_closest"] = bool(out["any_k1"]["median_ms"] <= out["closest_k1"]["median_ms"])
    print(json.dumps(out), flush=True)
s.close()
ctx.close()
