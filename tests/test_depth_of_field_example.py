"""examples/depth_of_field.cpp: the thin lens through the C++ facade (RayTracerScene::SetLens / GetLens) -- it compiles with g++ against
the C ABI, fails loudly without a GPU, and on the GPU every frame's PNG is the frame the Python mirror renders with the same lens."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, asset


def build_example(tmp_path):
    exe = str(tmp_path / "depth_of_field")
    lib_dir = os.path.join(ROOT, "raytracerwin_amd")
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "depth_of_field.cpp"),
                           "-L" + lib_dir, "-lrtwin", "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def test_depth_of_field_compiles_links_and_refuses_to_run_without_a_gpu(tmp_path):
    import torch
    exe = build_example(tmp_path)
    if torch.cuda.is_available():
        return          # what it renders is test_focus_pull_frames_equal_the_python_mirrors
    r = subprocess.run([exe, asset("TorusKnot.obj"), "32", "32", "2", "1", "3", str(tmp_path / "f")], capture_output=True, text=True)
    assert r.returncode == 1 and "no HIP device" in r.stderr


@pytest.mark.gpu
def test_focus_pull_frames_equal_the_python_mirrors(tmp_path):
    import raytracerwin_amd as R
    from PIL import Image
    exe = build_example(tmp_path)
    W, H, n_frames, passes, depth = 96, 54, 3, 2, 3
    out = subprocess.run([exe, asset("TorusKnot.obj"), str(W), str(H), str(n_frames), str(passes), str(depth), str(tmp_path / "f")],
                         capture_output=True, text=True, check=True).stdout
    focus = [float(m) for m in re.findall(r"focus (\S+) ->", out)]
    assert len(focus) == n_frames and focus == sorted(focus) and len(set(focus)) == n_frames
    ctx = R.Context(0)
    s = R.RayTracerScene(ctx)
    s.AddShape(R.RPlane.Create((0, 1, 0), (0, -2, 0)), R.SurfaceMaterial_DiffuseChecker((1, 1, 1), 2.0))
    s.AddShape(R.RMeshShape.Create(asset("TorusKnot.obj")), R.SurfaceMaterial_Diffuse((1.0, 0.9, 0.8)))
    s.set_camera(R.Camera.look_at((0, 1.5, 7), (0, 0, 0), (0, 1, 0), 45.0))
    fb = R.Framebuffer(ctx, W, H)
    frames = []
    for k, d in enumerate(focus):
        s.set_lens(R.Lens(0.15, d))
        fb.clear()
        for p in range(passes):
            R.ThreadWorker_Render(s, fb, 0, W * H - 1, depth, None, p, 4, 12345)
        argb = fb.resolve_argb()
        im = np.asarray(Image.open(str(tmp_path / ("f_%03d.png" % k)))).astype(np.uint32)
        assert im.shape == (H, W, 3)
        assert ((im[..., 0] << 16 | im[..., 1] << 8 | im[..., 2]).ravel() == (argb & 0xFFFFFF)).all(), k
        frames.append(argb)
    assert not (frames[0] == frames[1]).all() and not (frames[1] == frames[2]).all() and len(np.unique(frames[0])) > 50
    ctx.close()
