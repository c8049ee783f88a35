"""rtw_render_lighting on the CPU: tests/cpu_emul/lighting_main.cpp -- a stand-alone program over the C ABI, linked against the product's own sources
on the HIP stand-in under AddressSanitizer + UBSan, run directly (nothing preloaded) -- renders a 24 x 13 frame of TorusKnot and of the multi-shape
scene under both "lighting_deal" values; every dump must equal the model of tests/lighting_support.py over the dumped features bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ASSETS, ROOT, asset

import raytracerwin_amd as R
import camera_support as CS
import lighting_support as LS

W, H = 24, 13
LIGHTS = [(0, 1, (-3.0, 3.0, 2.0), (8.0, 6.0, 4.0), 0.5), (1, 0, (0.0, 0.8, 0.6), (0.5, 0.6, 0.7), 0.0)]      # lighting_main.cpp's


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    here = os.path.join(ROOT, "tests", "cpu_emul")
    subprocess.check_call(["make", "-C", here, "-f", "lighting.mk", "-j4"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    out = tmp_path_factory.mktemp("lighting_emul")
    # the program carries the sanitizers' runtime itself (lighting.mk links it statically): the inherited environment, plus their options
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(here, "_build", "lighting_main"), ASSETS, str(out)], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0 and "lighting_main ok: 4 frames" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    return out


@pytest.mark.parametrize("deal", [0, 1])
@pytest.mark.parametrize("tag", ["torus", "mixed"])
def test_emulated_lighting_equals_the_model(dumps, oracle_mod, tag, deal):
    feats = (np.fromfile(dumps / (tag + ".geom"), np.float32).reshape(-1, 4), np.fromfile(dumps / (tag + ".albedo"), np.float32).reshape(-1, 4),
             np.fromfile(dumps / (tag + ".ids"), np.int32).reshape(-1, 2))
    cam = np.fromfile(dumps / (tag + ".cam"), np.float32)
    accum = np.fromfile(dumps / ("%s_d%d.accum" % (tag, deal)), np.float32).reshape(-1, 4)
    argb = np.fromfile(dumps / ("%s_d%d.argb" % (tag, deal)), np.uint32)
    want = LS.model(R, CS.oracle_scene(oracle_mod, CS.SCENES[tag], asset), feats, cam, W, H, LIGHTS, np.float32(1e-3), 3, LS.ALBEDO, 0, 2, 9,
                    R.api.gamma_thresholds())
    assert want[2] == (True, True, True), want[2]       # something is lit, something shadowed, something culled
    assert (CS.bits(accum) == CS.bits(want[0])).all() and (argb == want[1]).all()
