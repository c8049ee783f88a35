"""examples/visibility.cpp: the device-buffer queries through the C++ facade (RayTracerScene::FindIntersectionsDevice / OccludedDevice) -- it
compiles with g++ against the C ABI, fails loudly without a GPU, and on the GPU its three counts (sky, lit, shadowed) are the ones the same
computation gives through the Python API."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, asset

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def build_visibility(tmp_path):
    exe = str(tmp_path / "visibility")
    lib_dir = os.path.join(ROOT, "raytracerwin_amd")
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROCM, "include"),
                           os.path.join(ROOT, "examples", "visibility.cpp"), "-L" + lib_dir, "-lrtwin", "-L" + os.path.join(ROCM, "lib"), "-lamdhip64",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath," + os.path.join(ROCM, "lib"), "-o", exe])
    return exe


def test_visibility_compiles_links_and_refuses_to_run_without_a_gpu(tmp_path):
    import torch
    exe = build_visibility(tmp_path)
    if torch.cuda.is_available():
        return          # what it computes is test_visibility_counts_equal_the_python_api
    r = subprocess.run([exe, asset("TorusKnot.obj"), "32", "32", str(tmp_path / "v.png")], capture_output=True, text=True)
    assert r.returncode == 1 and "no HIP device" in r.stderr


@pytest.mark.gpu
def test_visibility_counts_equal_the_python_api(tmp_path):
    import torch
    import raytracerwin_amd as R
    from PIL import Image
    exe = build_visibility(tmp_path)
    W, H = 96, 54
    png = str(tmp_path / "v.png")
    out = subprocess.run([exe, asset("TorusKnot.obj"), str(W), str(H), png], capture_output=True, text=True, check=True).stdout
    sky, lit, shadowed = [int(v) for v in re.search(r"sky (\d+) lit (\d+) shadowed (\d+)", out).groups()]
    assert sky + lit + shadowed == W * H and lit > 0 and shadowed > 0 and sky > 0
    ctx = R.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    s = R.RayTracerScene(ctx)
    s.AddShape(R.RPlane.Create((0, 1, 0), (0, -2, 0)), R.SurfaceMaterial_DiffuseChecker((1, 1, 1), 2.0))
    s.AddShape(R.RMeshShape.Create(asset("TorusKnot.obj")), R.SurfaceMaterial_Diffuse((1.0, 0.9, 0.8)))
    s.commit()
    rays = R.camera_rays(s.get_camera(), W, H, np.arange(W * H, dtype=np.int32), 0, 0, 12345)
    hits, shape, _ = s.trace_closest(torch.from_numpy(np.ascontiguousarray(rays, np.float32)).cuda(), tri=False)
    torch.cuda.synchronize()
    hits, shape = hits.cpu().numpy(), shape.cpu().numpy()
    # the example's float operations, one by one
    h = hits[shape >= 0]
    o = h[:, 0:3] + h[:, 3:6] * np.float32(1e-3)
    d = np.array([4.0, 6.0, 5.0], np.float32) - o
    ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    shadow = np.concatenate([o, d / ln[:, None], ln[:, None]], axis=1).astype(np.float32)
    occ = s.trace_occluded(torch.from_numpy(np.ascontiguousarray(shadow)).cuda())
    torch.cuda.synchronize()
    occ = occ.cpu().numpy()
    assert (sky, lit, shadowed) == (int((shape < 0).sum()), int((occ == 0).sum()), int((occ == 1).sum()))
    im = np.asarray(Image.open(png))
    assert im.shape[:2] == (H, W) and len(np.unique(im.reshape(H * W, -1), axis=0)) == 3
    ctx.close()
