"""rtw_reproject through both variants of rtw_reproject_kernels.h on the CPU: tests/cpu_emul/reproject_main.cpp -- a stand-alone program over the C ABI,
linked against the product's own sources on the HIP stand-in under AddressSanitizer + UBSan, run directly (nothing preloaded) -- reprojects three
frames under three camera pairs with the taps read directly and staged, and tries every refusal; the dumps must match the float64 reference and each
other bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import reproject_support as RS

BOUND = 1.044e-04       # tests/test_reproject_gpu.py: 8 x the float32 NumPy evaluation's own error (profiles/reproject_experiments.md section 1)
NAMES = ("accum", "geom", "albedo", "ids")


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    here = os.path.join(ROOT, "tests", "cpu_emul")
    subprocess.check_call(["make", "-C", here, "-f", "reproject.mk", "-j4"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    out = tmp_path_factory.mktemp("reproject_emul")
    for W, H, pair, _ in RS.EMUL_CASES:
        cc, cp, cleared = RS.PAIRS[pair]
        base = "%dx%d_%s" % (W, H, pair)
        np.array([W, H], np.int32).tofile(out / (base + ".size"))
        np.concatenate([cc, cp]).tofile(out / (base + ".cams"))
        for which, arrays in zip(("cur", "hist"), RS.inputs(W, H, cc, cp, cleared)):
            for a, name in zip(arrays, NAMES):
                a.tofile(out / ("%s.%s_%s" % (base, which, name)))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(here, "_build", "reproject_main"), str(out)] + ["%dx%d_%s" % c[:3] for c in RS.EMUL_CASES], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0 and "reproject_main ok: 18 dumps, refusals checked" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    return out


@pytest.mark.parametrize("W,H,pair,params", RS.EMUL_CASES, ids=lambda v: str(v) if not isinstance(v, tuple) else "defaults")
def test_emulated_reproject_equals_the_formula_under_both_variants(dumps, W, H, pair, params):
    from raytracerwin_amd import api
    got = [[np.fromfile(dumps / ("%dx%d_%s_s%d.%s" % (W, H, pair, s, kind)), dt) for kind, dt in (("accum", np.float32), ("argb", np.uint32))] for s in (0, 1)]
    cc, cp, cleared = RS.PAIRS[pair]
    cur, hist = RS.inputs(W, H, cc, cp, cleared)
    ref_sum, ref_n, margin = RS.reference(cc, cp, cur, hist, params)
    compared, share = RS.excluded(margin, cur)
    accum = got[0][0].reshape(H, W, 4)
    n = accum[..., 3].astype(np.int64)
    err = RS.error(accum[..., :3], n, ref_sum, ref_n, compared)
    print("error %.3e of bound %.3e, excluded %.4f" % (err, BOUND, share))
    assert share <= 0.03 and err <= BOUND and (n == ref_n)[compared].all()
    with np.errstate(all="ignore"):
        assert (got[0][1] == RS.pack(api.gamma_thresholds(), (accum[..., :3] / accum[..., 3:]).reshape(-1, 3))).all()
    assert (got[0][0].view(np.uint32) == got[1][0].view(np.uint32)).all() and (got[0][1] == got[1][1]).all()
