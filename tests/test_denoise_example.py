"""examples/denoise.cpp: the denoiser through the C++ facade (Denoise of RayTracerWin.hpp) -- it compiles with g++ against the C ABI, fails loudly
without a GPU, and on the GPU writes the one-pass frame and a filtered frame that is smoother than it."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, asset


def build_example(tmp_path):
    exe = str(tmp_path / "denoise")
    lib_dir = os.path.join(ROOT, "raytracerwin_amd")
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "denoise.cpp"),
                           "-L" + lib_dir, "-lrtwin", "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def test_denoise_example_compiles_links_and_refuses_to_run_without_a_gpu(tmp_path):
    import torch
    exe = build_example(tmp_path)
    if torch.cuda.is_available():
        return          # what it writes is test_the_denoised_image_is_smoother
    r = subprocess.run([exe, asset("unitychan.obj"), "32", "32", str(tmp_path / "d")], capture_output=True, text=True)
    assert r.returncode == 1 and "no HIP device" in r.stderr


@pytest.mark.gpu
def test_the_denoised_image_is_smoother(tmp_path):
    from PIL import Image
    subprocess.run([build_example(tmp_path), asset("unitychan.obj"), "96", "54", str(tmp_path / "d")], check=True)
    noisy, clean = (np.asarray(Image.open(str(tmp_path / ("d_%s.png" % k)))).astype(np.float64)[..., :3] for k in ("noisy", "denoised"))
    rough = lambda im: np.abs(np.diff(im, axis=1)).mean()        # noqa: E731  mean step between horizontal neighbours
    assert noisy.shape == clean.shape == (54, 96, 3) and 0 < rough(clean) < 0.8 * rough(noisy)
