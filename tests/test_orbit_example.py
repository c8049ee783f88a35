"""examples/orbit.cpp: the settable camera through the C++ facade (RayTracerScene::SetCamera / GetCamera) -- it compiles with g++
against the C ABI, fails loudly without a GPU, and on the GPU every view's PNG is the frame the Python mirror renders from that eye."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, asset


def build_orbit(tmp_path):
    exe = str(tmp_path / "orbit")
    lib_dir = os.path.join(ROOT, "raytracerwin_amd")
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "orbit.cpp"),
                           "-L" + lib_dir, "-lrtwin", "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def test_orbit_compiles_links_and_refuses_to_run_without_a_gpu(tmp_path):
    import torch
    exe = build_orbit(tmp_path)
    if torch.cuda.is_available():
        return          # what it renders is test_orbit_views_equal_the_python_mirrors
    r = subprocess.run([exe, asset("TorusKnot.obj"), "32", "32", "2", "1", "3", str(tmp_path / "v")], capture_output=True, text=True)
    assert r.returncode == 1 and "no HIP device" in r.stderr


@pytest.mark.gpu
def test_orbit_views_equal_the_python_mirrors(tmp_path):
    import raytracerwin_amd as R
    from PIL import Image
    exe = build_orbit(tmp_path)
    W, H, views, passes, depth = 96, 54, 3, 2, 3
    out = subprocess.run([exe, asset("TorusKnot.obj"), str(W), str(H), str(views), str(passes), str(depth), str(tmp_path / "v")],
                         capture_output=True, text=True, check=True).stdout
    eyes = [tuple(float(v) for v in m) for m in re.findall(r"eye (\S+) (\S+) (\S+) ->", out)]
    assert len(eyes) == views and len(set(eyes)) == views
    ctx = R.Context(0)
    s = R.RayTracerScene(ctx)
    s.AddShape(R.RPlane.Create((0, 1, 0), (0, -2, 0)), R.SurfaceMaterial_DiffuseChecker((1, 1, 1), 2.0))
    s.AddShape(R.RMeshShape.Create(asset("TorusKnot.obj")), R.SurfaceMaterial_Diffuse((1.0, 0.9, 0.8)))
    fb = R.Framebuffer(ctx, W, H)
    frames = []
    for v, eye in enumerate(eyes):
        s.set_camera(R.Camera.look_at(eye, (0, 0, 0), (0, 1, 0), 45.0))
        fb.clear()
        for p in range(passes):
            R.ThreadWorker_Render(s, fb, 0, W * H - 1, depth, None, p, 4, 12345)
        argb = fb.resolve_argb()
        im = np.asarray(Image.open(str(tmp_path / ("v_%03d.png" % v)))).astype(np.uint32)
        assert im.shape == (H, W, 3)
        assert ((im[..., 0] << 16 | im[..., 1] << 8 | im[..., 2]).ravel() == (argb & 0xFFFFFF)).all(), v
        frames.append(argb)
    assert not (frames[0] == frames[1]).all() and len(np.unique(frames[0])) > 50
    ctx.close()
