"""rtw_denoise through every kernel of rtw_denoise_kernels.h on the CPU: tests/cpu_emul/denoise_main.cpp -- a stand-alone program over the C ABI,
linked against the product's own sources on the HIP stand-in under AddressSanitizer + UBSan, run directly (nothing preloaded) -- filters three
frames at 5 and 6 levels under both tilings and tries every refusal; the dumps must match the float64 reference and each other bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import denoise_support as DS

BOUND = 1.706e-06       # tests/test_denoise_gpu.py: 8 x the float32 NumPy evaluation's own error (profiles/denoise_experiments.md section 1)
FRAMES = [(5, 3), (37, 23), (131, 70)]


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    here = os.path.join(ROOT, "tests", "cpu_emul")
    subprocess.check_call(["make", "-C", here, "-f", "denoise.mk", "-j4"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    out = tmp_path_factory.mktemp("denoise_emul")
    for W, H in FRAMES:
        for a, name in zip(DS.inputs(W, H), ("accum", "geom", "albedo", "ids")):
            a.tofile(out / ("%dx%d.%s" % (W, H, name)))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(here, "_build", "denoise_main"), str(out)] + [str(v) for f in FRAMES for v in f], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0 and "denoise_main ok: 12 dumps, refusals checked" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    return out


@pytest.mark.parametrize("levels", [5, 6])
@pytest.mark.parametrize("W,H", FRAMES)
def test_emulated_denoise_equals_the_formula_under_both_tilings(dumps, W, H, levels):
    from raytracerwin_amd import api
    got = [[np.fromfile(dumps / ("%dx%d_l%d_t%d.%s" % (W, H, levels, t, kind)), dt) for kind, dt in (("accum", np.float32), ("argb", np.uint32))] for t in (0, 1)]
    accum = got[0][0].reshape(H, W, 4)
    err = DS.error(accum[..., :3], DS.reference(*DS.inputs(W, H), (levels,) + DS.DEFAULTS[1:]))
    print("error %.3e of bound %.3e" % (err, BOUND))
    assert err <= BOUND and (accum[..., 3] == 1).all()
    assert (got[0][1] == DS.pack(api.gamma_thresholds(), accum[..., :3].reshape(-1, 3))).all()
    assert (got[0][0].view(np.uint32) == got[1][0].view(np.uint32)).all() and (got[0][1] == got[1][1]).all()
