"""examples/adaptive.cpp: per-pixel pass budgets through the C++ facade (SampleBudget, RayTracerScene::RenderPassesBudget of RayTracerWin.hpp) -- it
compiles with g++ against the C ABI, fails loudly without a GPU, and on the GPU spends fewer pixel passes than a uniform render and writes its image."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, asset

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def build_example(tmp_path):
    exe, lib_dir = str(tmp_path / "adaptive"), os.path.join(ROOT, "raytracerwin_amd")
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROCM, "include"),
                           os.path.join(ROOT, "examples", "adaptive.cpp"), "-L" + lib_dir, "-lrtwin", "-L" + os.path.join(ROCM, "lib"), "-lamdhip64",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath," + os.path.join(ROCM, "lib"), "-o", exe])
    return exe


def test_adaptive_example_compiles_links_and_refuses_to_run_without_a_gpu(tmp_path):
    import torch
    exe = build_example(tmp_path)
    if torch.cuda.is_available():
        return          # what it does is test_adaptive_rounds_spend_less_than_uniform
    r = subprocess.run([exe, asset("TorusKnot.obj"), "32", "32", "1", str(tmp_path / "a.png")], capture_output=True, text=True)
    assert r.returncode == 1 and "no HIP device" in r.stderr


@pytest.mark.gpu
def test_adaptive_rounds_spend_less_than_uniform(tmp_path):
    from PIL import Image
    png = str(tmp_path / "a.png")
    out = subprocess.run([build_example(tmp_path), asset("TorusKnot.obj"), "96", "54", "2", png], capture_output=True, text=True, check=True).stdout
    spent, uniform = [int(v) for v in re.search(r"spent (\d+) pixel passes, a uniform render of the same depth (\d+)", out).groups()]
    assert 96 * 54 * 4 < spent < uniform and uniform == 96 * 54 * 36
    im = np.asarray(Image.open(png)).astype(np.float64)[..., :3]
    assert im.shape == (54, 96, 3) and im.std() > 1
