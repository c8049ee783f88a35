"""examples/svgf.cpp: the whole chain through the C++ facade (ReprojectMoments, DenoiseVariance of RayTracerWin.hpp) -- it compiles with g++ against
the C ABI, fails loudly without a GPU, and on the GPU writes its PNG pairs."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, asset


def build_example(tmp_path):
    exe, lib_dir = str(tmp_path / "svgf"), os.path.join(ROOT, "raytracerwin_amd")
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "svgf.cpp"),
                           "-L" + lib_dir, "-lrtwin", "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def test_svgf_example_compiles_links_and_refuses_to_run_without_a_gpu(tmp_path):
    import torch
    exe = build_example(tmp_path)
    if torch.cuda.is_available():
        return          # what it writes is test_the_chain_writes_its_frames
    r = subprocess.run([exe, asset("unitychan.obj"), "32", "32", "2", str(tmp_path / "t")], capture_output=True, text=True)
    assert r.returncode == 1 and "no HIP device" in r.stderr


@pytest.mark.gpu
def test_the_chain_writes_its_frames(tmp_path):
    from PIL import Image
    subprocess.run([build_example(tmp_path), asset("unitychan.obj"), "96", "54", "4", str(tmp_path / "t")], check=True)
    load = lambda k, kind: np.asarray(Image.open(str(tmp_path / ("t_%03d_%s.png" % (k, kind))))).astype(np.float64)[..., :3]      # noqa: E731
    svgf, fixed = load(3, "svgf"), load(3, "fixed")
    assert svgf.shape == (54, 96, 3) and svgf.std() > 1 and 0 < np.abs(svgf - fixed).mean() < 40       # an image, and not the fixed filter's
