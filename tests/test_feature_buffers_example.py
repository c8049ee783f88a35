"""examples/feature_buffers.cpp: the feature buffers through the C++ facade (FeatureBuffers / RayTracerScene::RenderFeatures) -- it compiles with
g++ against the C ABI, fails loudly without a GPU, and on the GPU its three PNGs are the images the Python mirror makes of the same buffers."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, asset

import scenes as SC


def build_example(tmp_path):
    exe = str(tmp_path / "feature_buffers")
    lib_dir = os.path.join(ROOT, "raytracerwin_amd")
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "feature_buffers.cpp"),
                           "-L" + lib_dir, "-lrtwin", "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def test_feature_buffers_compiles_links_and_refuses_to_run_without_a_gpu(tmp_path):
    import torch
    exe = build_example(tmp_path)
    if torch.cuda.is_available():
        return          # what it writes is test_the_three_images_equal_the_python_mirrors
    r = subprocess.run([exe, asset("unitychan.obj"), "32", "32", "1", str(tmp_path / "f")], capture_output=True, text=True)
    assert r.returncode == 1 and "no HIP device" in r.stderr


def rgb_words(path):
    from PIL import Image
    im = np.asarray(Image.open(path)).astype(np.uint32)
    return (im[..., 0] << 16 | im[..., 1] << 8 | im[..., 2]).ravel()


def byte(t):
    return np.clip((t.astype(np.float32) * np.float32(255.0) + np.float32(0.5)).astype(np.float32).astype(np.int32), 0, 255).astype(np.uint32)


@pytest.mark.gpu
def test_the_three_images_equal_the_python_mirrors(tmp_path, oracle_mod):
    import raytracerwin_amd as R
    import features_support as FS
    exe = build_example(tmp_path)
    W, H, passes = 96, 54, 2
    out = subprocess.run([exe, asset("unitychan.obj"), str(W), str(H), str(passes), str(tmp_path / "f")], capture_output=True, text=True, check=True).stdout
    m = re.search(r"(\d+) of (\d+) pixels hit something; distances (\S+) \.\. (\S+)", out)
    assert m and int(m.group(2)) == W * H
    ctx = R.Context(0)
    s = FS.product_scene(R, oracle_mod, ctx, SC.default_scene(True), asset)
    fb = R.FeatureBuffers(ctx, W, H)
    s.render_features(fb, 10, 0, 1, 0, passes, 4, 12345)
    depth, normal, color = fb.means()
    ids = fb.read()[2]
    hit = ids[:, 0] >= 0
    assert int(m.group(1)) == int(hit.sum()) and 0 < hit.sum() < W * H
    near, far = depth[hit].min(), depth[hit].max()
    assert np.float32(float(m.group(3))) == near and np.float32(float(m.group(4))) == far and near < far
    assert (rgb_words(str(tmp_path / "f_albedo.png")) == (oracle_mod.make_pixel_colors(color) & 0xFFFFFF)).all()
    n = byte(normal * np.float32(0.5) + np.float32(0.5))
    assert (rgb_words(str(tmp_path / "f_normal.png")) == (n[:, 0] << 16 | n[:, 1] << 8 | n[:, 2])).all()
    g = np.where(hit, byte((far - depth) / (far - near)), 0).astype(np.uint32)
    assert (rgb_words(str(tmp_path / "f_depth.png")) == (g << 16 | g << 8 | g)).all()
    assert len(np.unique(g)) > 20 and len(np.unique(n[:, 0])) > 20
    ctx.close()
