"""examples/temporal.cpp: reprojection through the C++ facade (Reproject of RayTracerWin.hpp) -- it compiles with g++ against the C ABI, fails loudly
without a GPU, and on the GPU writes its PNG pairs, the accumulated frame closer to the frames before it than the single-sample one."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, asset


def build_example(tmp_path):
    exe = str(tmp_path / "temporal")
    lib_dir = os.path.join(ROOT, "raytracerwin_amd")
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "temporal.cpp"),
                           "-L" + lib_dir, "-lrtwin", "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def test_temporal_example_compiles_links_and_refuses_to_run_without_a_gpu(tmp_path):
    import torch
    exe = build_example(tmp_path)
    if torch.cuda.is_available():
        return          # what it writes is test_history_steadies_the_frames
    r = subprocess.run([exe, asset("unitychan.obj"), "32", "32", "2", str(tmp_path / "t")], capture_output=True, text=True)
    assert r.returncode == 1 and "no HIP device" in r.stderr


@pytest.mark.gpu
def test_history_steadies_the_frames(tmp_path):
    from PIL import Image
    subprocess.run([build_example(tmp_path), asset("unitychan.obj"), "96", "54", "6", str(tmp_path / "t")], check=True)
    load = lambda k, kind: np.asarray(Image.open(str(tmp_path / ("t_%03d_%s.png" % (k, kind))))).astype(np.float64)[..., :3]      # noqa: E731
    flicker = lambda kind: np.abs(load(5, kind) - load(4, kind)).mean()        # noqa: E731  mean change between two successive frames
    assert load(5, "temporal").shape == (54, 96, 3) and 0 < flicker("temporal") < 0.8 * flicker("single")
