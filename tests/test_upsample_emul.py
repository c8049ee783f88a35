"""rtw_upsample through the kernels of rtw_upsample_kernels.h on the CPU: tests/cpu_emul/upsample_main.cpp -- a stand-alone program over the C ABI,
linked against the product's own sources on the HIP stand-in under AddressSanitizer + UBSan, run directly (nothing preloaded) -- runs three frames
under both stagings; the dumps must match the float64 reference and each other bit for bit.

Figures: the emulation's largest error over the three frames is 1.140e-07 (74x46 from 37x23) of the bound 2.685e-05."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import upsample_support as US

BOUND = 2.685e-05       # 8 x the largest float32-vs-float64 NumPy error over US.CASES (3.356e-06, 74x46 from 37x23 with sigmas 0.05 / 0.01)
NAMES = ("lo_accum", "lo_geom", "lo_albedo", "lo_ids", "hi_geom", "hi_albedo", "hi_ids")


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    here = os.path.join(ROOT, "tests", "cpu_emul")
    subprocess.check_call(["make", "-C", here, "-f", "upsample.mk", "-j4"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    out = tmp_path_factory.mktemp("upsample_emul")
    for W, H, w, h, _ in US.EMUL_CASES:
        lo, f_hi = US.inputs(W, H, w, h)
        for name, a in zip(NAMES, lo + f_hi):
            a.tofile(out / ("%dx%d.%s" % (W, H, name)))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(here, "_build", "upsample_main"), str(out)] + [str(v) for c in US.EMUL_CASES for v in c[:4]], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0 and "upsample_main ok: 6 dumps" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    return out


@pytest.mark.parametrize("W,H,w,h,params", US.EMUL_CASES, ids=lambda v: "x".join("%g" % x for x in v) if isinstance(v, tuple) else str(v))
def test_emulated_upsample_equals_the_formula_under_both_stagings(dumps, W, H, w, h, params):
    from raytracerwin_amd import api
    got = [[np.fromfile(dumps / ("%dx%d_s%d.%s" % (W, H, v, k)), dt) for k, dt in (("accum", np.float32), ("argb", np.uint32))] for v in (0, 1)]
    accum = got[0][0].reshape(H, W, 4)
    ref, count, rounds, margin = US.reference(*US.inputs(W, H, w, h), params)
    keep, share = US.compared(rounds, margin)
    err = US.error(accum[..., :3], ref, keep)
    print("error %.3e of bound %.3e, excluded %.4f" % (err, BOUND, share))
    assert share <= US.CAP and err <= BOUND and (accum[..., 3] == count)[keep].all()
    assert (got[0][1] == US.pack(api.gamma_thresholds(), accum[..., :3].reshape(-1, 3))).all()
    for a, b in zip(got[0], got[1]):
        assert (a.view(np.uint32) == b.view(np.uint32)).all()


def test_the_inputs_reach_every_round():
    """from the references alone, over the cases together: each round decides some non-empty pixel and round 1 at least half of them, within the cap
    of excluded pixels in every case -- so the bound cannot be met by a kernel that lacks the fallback rounds"""
    n = np.zeros(4, np.int64)
    for W, H, w, h, params in US.CASES:
        _, _, rounds, margin = US.reference(*US.inputs(W, H, w, h), params)
        assert US.compared(rounds, margin)[1] <= US.CAP
        n += np.bincount(rounds.ravel(), minlength=4)
    assert n[1] >= 1 and n[2] >= 1 and n[3] >= 1 and 2 * n[1] >= n[1:].sum()
