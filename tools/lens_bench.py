#!/usr/bin/env python3
"""tools/lens_bench.py CONFIG K [RADIUS]  -- ON THE GPU BOX: same-session A/B of the two lens routes of pipeline 4 ("lens_route" 0 =
gprimary_kernel's LENS instantiation, 1 = the camera round through glens_kernel) against the pinhole frame of the same scene, in the
style of tools/ab.py: per set 3 warm-up calls and 12 timed rtw_render_passes calls of K passes (HIP-synchronised wall clock per
call), the sets interleaved twice; prints median / min ms per pass and each lens route's cost relative to the pinhole.
The lens: radius RADIUS (0.15), focused on the centre of the scene's last mesh from the reference's eye.  CONFIG as bench.CONFIGS."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import raytracerwin_amd as R  # noqa: E402
import bench  # noqa: E402

cfg, K = sys.argv[1], int(sys.argv[2])
radius = float(sys.argv[3]) if len(sys.argv) > 3 else 0.15
mesh, W, H, spp, depth, kind = bench.CONFIGS[cfg]
ctx = R.Context(0)
s = R.RayTracerScene(ctx)
if kind == "setup":
    from raytracerwin_amd.setup_scene import SetupScene
    SetupScene(s, os.path.join(ROOT, "assets", mesh + ".obj"))
else:
    s.AddShape(R.RMeshShape.Create(os.path.join(ROOT, "assets", mesh + ".obj")), bench.make_material(R, kind))
s.commit()
b = s.mesh_info(s.n_shapes - 1)["bounds"]
centre = 0.5 * (b[:3] + b[3:])
cam = s.get_camera().as_array()
focus = float(np.dot(centre - cam[0:3], cam[9:12]))         # measured along `forward`
lens = R.Lens(radius, focus)
fb = R.Framebuffer(ctx, W, H)
SETS = [("pinhole", None, -1), ("lens, route 0 (gprimary_kernel)", lens, 0), ("lens, route 1 (camera round)", lens, 1)]
res = {name: [] for name, _, _ in SETS}
for rnd in range(2):          # the sets interleaved, twice: drift of the box's clock shows as a difference between the rounds
    for name, ln, route in SETS:
        s.set_lens(ln)
        ctx.set_option("lens_route", route)
        s.render_reserve(fb, 10, 0, 1, depth, K, spp)
        p = 0
        for i in range(3):
            s.render_passes(fb, 10, 0, 1, depth, None, p, K, spp, 12345); p += K
        ctx.synchronize()
        for i in range(12):
            t0 = time.perf_counter()
            s.render_passes(fb, 10, 0, 1, depth, None, p, K, spp, 12345); p += K
            ctx.synchronize()
            res[name].append((time.perf_counter() - t0) * 1e3 / K)
ctx.set_option("lens_route", -1)
base = np.median(np.array(res["pinhole"]))
print("%s K=%d %dx%d %d spp depth %d, lens radius %g focus %.4f" % (cfg, K, W, H, spp, depth, radius, focus))
for name, _, _ in SETS:
    a = np.array(res[name])
    print("  %-34s median %.4f  min %.4f  (rounds %.4f / %.4f) ms per pass   x %.2f of the pinhole" % (name, np.median(a), a.min(), np.median(a[:12]), np.median(a[12:]), np.median(a) / base))
