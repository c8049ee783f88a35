"""examples/lighting.cpp: direct lighting through the C++ facade (RayTracerScene::RenderLighting of RayTracerWin.hpp) -- it compiles with g++ against
the C ABI, fails loudly without a GPU, and on the GPU writes a hard-shadow frame with lit and unlit surface in it and a soft-shadow frame that differs."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, asset


def build_example(tmp_path):
    exe = str(tmp_path / "lighting")
    lib_dir = os.path.join(ROOT, "raytracerwin_amd")
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "lighting.cpp"),
                           "-L" + lib_dir, "-lrtwin", "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def test_lighting_example_compiles_links_and_refuses_to_run_without_a_gpu(tmp_path):
    import torch
    exe = build_example(tmp_path)
    if torch.cuda.is_available():
        return          # what it writes is test_the_light_casts_hard_and_soft_shadows
    r = subprocess.run([exe, asset("unitychan.obj"), "32", "32", str(tmp_path / "l")], capture_output=True, text=True)
    assert r.returncode == 1 and "no HIP device" in r.stderr


@pytest.mark.gpu
def test_the_light_casts_hard_and_soft_shadows(tmp_path):
    from PIL import Image
    subprocess.run([build_example(tmp_path), asset("unitychan.obj"), "96", "54", str(tmp_path / "l"), "0.5"], check=True)
    hard, soft = (np.asarray(Image.open(str(tmp_path / ("l_%s.png" % k)))).astype(np.float64)[..., :3] for k in ("hard", "soft"))
    assert hard.shape == soft.shape == (54, 96, 3)
    assert (hard.max(axis=2) == 0).any() and (hard.max(axis=2) > 64).any()       # surface the light does not reach, surface it does
    assert (hard != soft).any()
