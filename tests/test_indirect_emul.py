"""The two programs that go with rtw_render_indirect, compiled and run.  tests/cpu_emul/indirect_main.cpp, stand-alone on the HIP stand-in under ASan + UBSan
(nothing preloaded), compares both deals and the unstaged blocks on two 24 x 13 frames; its dump must equal tests/indirect_support.py's model bit for bit.
examples/indirect.cpp compiles with g++ against the C ABI, fails loudly without a GPU, and with one writes a direct, an indirect and a summed frame."""
import os
import subprocess

import numpy as np

from conftest import ASSETS, ROOT, asset

import raytracerwin_amd as R
import camera_support as CS
import indirect_support as IS

LIGHTS = [(0, 1, (-3.0, 3.0, 2.0), (8.0, 6.0, 4.0), 0.5), (1, 0, (0.0, 0.8, 0.6), (0.5, 0.6, 0.7), 0.0)]      # indirect_main.cpp's
SCENES = {"torus": CS.TORUS, "mixed": CS.MIXED[:2] + CS.MIXED[3:]}      # indirect_main.cpp's


def test_emulated_indirect_equals_the_model(tmp_path, oracle_mod):
    here = os.path.join(ROOT, "tests", "cpu_emul")
    subprocess.check_call(["make", "-C", here, "-f", "indirect.mk", "-j4"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(here, "_build", "indirect_main"), ASSETS, str(tmp_path)], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0 and "indirect_main ok" in r.stdout and "runtime error" not in r.stderr, (r.stdout[-1500:], r.stderr[-3000:])
    for tag, shapes in SCENES.items():
        n, words = 24 * 13, np.fromfile(tmp_path / (tag + ".bin"), np.uint32)       # geom, albedo, ids, the camera's 13 floats, accum, argb
        geom, albedo, ids, cam, accum, argb = np.split(words, np.cumsum([4 * n, 4 * n, 2 * n, 13, 4 * n]))
        feats = (geom.view(np.float32).reshape(n, 4), albedo.view(np.float32).reshape(n, 4), ids.view(np.int32).reshape(n, 2))
        want = IS.model(R, CS.oracle_scene(oracle_mod, shapes, asset), feats, cam.view(np.float32), 24, 13, LIGHTS, np.float32(1e-3), 2, IS.ALBEDO, 0, 2, 9,
                        R.api.gamma_thresholds())
        # a gather miss, a lit hit, a shadowed hit (the few casting pixels of the torus frame have none: the multi-shape frame does), a culled light job
        assert want[2] == (True, True, tag == "mixed", True), (tag, want[2])
        assert (accum.reshape(n, 4) == CS.bits(want[0])).all() and (argb == want[1]).all(), tag


def test_indirect_example_compiles_and_lights_what_the_light_does_not_reach(tmp_path):
    import torch
    exe, lib_dir = str(tmp_path / "indirect"), os.path.join(ROOT, "raytracerwin_amd")
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "indirect.cpp"),
                           "-L" + lib_dir, "-lrtwin", "-Wl,-rpath," + lib_dir, "-o", exe])
    r = subprocess.run([exe, asset("unitychan.obj"), "96", "54", str(tmp_path / "i")], capture_output=True, text=True)
    if r.returncode == 1 and "no HIP device" in r.stderr:
        assert not torch.cuda.is_available()
        return
    from PIL import Image
    assert r.returncode == 0, r.stderr
    direct, indirect, both = (np.asarray(Image.open(str(tmp_path / ("i_%s.png" % k)))).astype(int)[..., :3] for k in ("direct", "indirect", "sum"))
    assert ((direct.max(axis=2) == 0) & (indirect.max(axis=2) > 0)).any()       # surface in shadow that its neighbourhood or the sky lights
    assert both.shape == (54, 96, 3) and (both >= np.maximum(direct, indirect)).all() and (both > direct).any()
