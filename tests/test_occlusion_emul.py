"""rtw_render_occlusion on the CPU: tests/cpu_emul/occlusion_main.cpp -- a stand-alone program over the C ABI, linked against the product's own sources
on the HIP stand-in under AddressSanitizer + UBSan, run directly (nothing preloaded) -- renders a 24 x 13 frame of TorusKnot and of the multi-shape
scene under both "occlusion_order" values; every dump must equal the model of tests/occlusion_support.py over the dumped features bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ASSETS, ROOT, asset

import raytracerwin_amd as R
import camera_support as CS
import occlusion_support as OS

W, H = 24, 13


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    here = os.path.join(ROOT, "tests", "cpu_emul")
    subprocess.check_call(["make", "-C", here, "-f", "occlusion.mk", "-j4"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    out = tmp_path_factory.mktemp("occlusion_emul")
    # the program carries the sanitizers' runtime itself (occlusion.mk links it statically): the inherited environment, plus their options
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(here, "_build", "occlusion_main"), ASSETS, str(out)], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0 and "occlusion_main ok: 4 frames" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    return out


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("tag", ["torus", "mixed"])
def test_emulated_occlusion_equals_the_model(dumps, oracle_mod, tag, order):
    feats = (np.fromfile(dumps / (tag + ".geom"), np.float32).reshape(-1, 4), np.fromfile(dumps / (tag + ".albedo"), np.float32).reshape(-1, 4),
             np.fromfile(dumps / (tag + ".ids"), np.int32).reshape(-1, 2))
    cam = np.fromfile(dumps / (tag + ".cam"), np.float32)
    accum = np.fromfile(dumps / ("%s_o%d.accum" % (tag, order)), np.float32).reshape(-1, 4)
    argb = np.fromfile(dumps / ("%s_o%d.argb" % (tag, order)), np.uint32)
    want = OS.model(R, CS.oracle_scene(oracle_mod, CS.SCENES[tag], asset), feats, cam, W, H, 0.5, np.float32(1e-3), 5, OS.COSINE, 0, 2, 9,
                    R.api.gamma_thresholds())
    assert (feats[2][:, 0] >= 0).any() and (CS.bits(accum) == CS.bits(want[0])).all() and (argb == want[1]).all()
    assert (accum[:, 0] < accum[:, 3]).any()           # something is occluded
