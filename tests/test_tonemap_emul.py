"""rtw_tonemap / rtw_exposure_meter on the CPU: tests/cpu_emul/tonemap_main.cpp -- a stand-alone program over the C ABI, linked against the product's own
sources on the HIP stand-in under AddressSanitizer + UBSan, run directly (nothing preloaded) -- runs every step of tests/tonemap_support.py's cases over
wrapped host arrays; every dump (destination accumulator and ARGB, exposure bits, frame count, histogram) must equal the NumPy model bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import raytracerwin_amd as R
import tonemap_support as TS


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    here = os.path.join(ROOT, "tests", "cpu_emul")
    subprocess.check_call(["make", "-C", here, "-f", "tonemap.mk", "-j4"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    out = tmp_path_factory.mktemp("tonemap_emul")
    fr, lines, first_step = TS.frames(), [], {}
    for tag, (_, _, acc) in fr.items():
        acc.tofile(out / (tag + ".acc"))
    for case, steps in TS.CASES.items():
        first_step[case] = len(lines)
        for k, (frame, mode, hist, blocks, kw) in enumerate(steps):
            p = dict(TS.DEFAULTS, **kw)
            lines.append("%d %s %d %d %s %d %d %d %.9g %.9g %.9g %.9g %.9g %.9g %.9g" % (
                k == 0, frame, fr[frame][0], fr[frame][1], mode, hist, blocks, p["curve"], p["key"], p["white"], p["low_fraction"], p["high_fraction"],
                p["min_exposure"], p["max_exposure"], p["adapt"]))
    (out / "steps.txt").write_text("\n".join(lines) + "\n")
    # the program carries the sanitizers' runtime itself (tonemap.mk links it statically): the inherited environment, plus their options
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(here, "_build", "tonemap_main"), str(out)], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0 and "tonemap_main ok: %d steps" % len(lines) in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    return out, first_step


@pytest.mark.parametrize("case", list(TS.CASES))
def test_emulated_tonemap_equals_the_model(dumps, case):
    out, first_step = dumps
    for k, want in enumerate(TS.expected(case, R.api.gamma_thresholds())):
        base = str(out / str(first_step[case] + k))
        st = np.fromfile(base + ".state", np.uint32)
        got = (st[0:1].view(np.float32)[0], int(st[1]), st[2:])
        assert TS.same(got, np.fromfile(base + ".accum", np.float32).reshape(-1, 4), np.fromfile(base + ".argb", np.uint32), want), (case, k, got[:2], want[0][:3])
