"""The thin lens through every touched kernel on the CPU: tests/cpu_emul/lens_main.cpp -- a stand-alone program over the C ABI, linked against
the product's own sources on the HIP stand-in under AddressSanitizer + UBSan, run directly (nothing preloaded) -- renders frames with a
lens through pipeline 4 (both lens routes), 3 and 0; its dumps must equal the oracle behind the lens-ray model (tests/lens_support.py) bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ASSETS, ROOT, asset

import raytracerwin_amd as R
import camera_support as CS
import lens_support as LS

DEPTH, RADIUS = 3, 0.2
# (pipeline, lens_route): pipeline 4 through gprimary_kernel's LENS instantiation and through the camera round, pipelines 3 and 0
ROUTES = [(4, 0), (4, 1), (3, -1), (0, -1)]
# (scene, pose, pipeline, lens_route, width, height, n_passes, sub_samples, radius, begin, end); radius < 0: no lens is ever set; begin < 0: whole frame
JOBS = [(sc, pose) + route + (96, 54, 2, 2, RADIUS, -1, -1) for sc in ("torus", "mixed") for pose in ("offaxis", "inside") for route in ROUTES]
JOBS += [("torus", "offaxis", 4, 1, 96, 54, 5, 1, RADIUS, -1, -1),           # five passes in one group
         ("mixed", "offaxis", 4, 1, 50, 37, 1, 2, RADIUS, -1, -1),           # a frame that does not tile into whole 64-pixel tiles
         ("mixed", "offaxis", 4, 0, 50, 37, 1, 2, RADIUS, -1, -1),
         ("mixed", "offaxis", 4, 1, 96, 54, 1, 2, RADIUS, 1000, 3000),       # a pixel range that starts and ends mid-row
         ("torus", "offaxis", 4, 0, 96, 54, 1, 2, RADIUS, 1000, 3000)]
PINHOLE = [("torus", "offaxis", 4, 1, 96, 54, 1, 2, 0.0, -1, -1), ("torus", "offaxis", 4, 1, 96, 54, 1, 2, -1.0, -1, -1)]      # radius 0 and never set


def job_name(j):
    return "%s_%s_p%d_r%d_%dx%d_k%d_s%d_a%g_%d_%d" % j


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    here = os.path.join(ROOT, "tests", "cpu_emul")
    subprocess.check_call(["make", "-C", here, "-f", "lens.mk", "-j4"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    out = tmp_path_factory.mktemp("lens_emul")
    lines = []
    for j in JOBS + PINHOLE:
        sc, pose, pipeline, route, W, H, npass, ns, radius, begin, end = j
        eye, target, up, vfov = CS.POSES[pose]
        lines.append(" ".join([job_name(j), sc] + [repr(float(v)) for v in eye + target + up] + [repr(float(vfov)), repr(float(radius)), repr(LS.target_distance(CS.POSES[pose]))] +
                              [str(v) for v in (pipeline, route, W, H, npass, ns, DEPTH, begin, end)]))
    jobs = out / "jobs.txt"
    jobs.write_text("\n".join(lines) + "\n")
    # the program carries the sanitizers' runtime itself (lens.mk links it statically): the inherited environment, plus their options
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(here, "_build", "lens_main"), ASSETS, str(out), str(jobs)], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0 and ("lens_main ok: %d frames" % len(JOBS + PINHOLE)) in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    report = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in (out / "report.txt").read_text().splitlines()}
    return out, report


def read(out, name, W, H):
    return np.fromfile(out / (name + ".accum"), np.float32).reshape(-1, 4), np.fromfile(out / (name + ".argb"), np.uint32)


@pytest.mark.parametrize("job", JOBS, ids=job_name)
def test_emulated_lens_frame_equals_the_oracle(dumps, oracle_mod, job):
    out, report = dumps
    sc, pose, pipeline, route, W, H, npass, ns, radius, begin, end = job
    name = job_name(job)
    lens = np.fromfile(out / (name + ".lens"), np.float32)
    assert lens[0] == np.float32(radius) and abs(float(lens[1]) - LS.target_distance(CS.POSES[pose])) < 1e-5
    ran, has_bins = report[name]
    assert has_bins == 0                                    # no mesh gets bins with a lens
    assert ran == pipeline, (ran, pipeline)                 # the pipeline asked for ran: no fallback
    want = LS.oracle_frame(oracle_mod, asset, CS.SCENES[sc], CS.cam13(R, pose), lens, W, H, ns, DEPTH, n_passes=npass,
                           begin=max(begin, 0), end=None if begin < 0 else end)
    accum, argb = read(out, name, W, H)
    assert (LS.bits(accum) == LS.bits(want[0])).all() and (argb == want[1]).all()


def test_emulated_radius_zero_is_the_pinhole(dumps, oracle_mod):
    out, report = dumps
    zero, never = (job_name(j) for j in PINHOLE)
    a0, b0 = read(out, zero, 96, 54)
    a1, b1 = read(out, never, 96, 54)
    assert (LS.bits(a0) == LS.bits(a1)).all() and (b0 == b1).all()
    assert report[zero] == [4, 1] and report[never] == [4, 1]          # pipeline 4 ran, and the bins are there
    want = CS.oracle_frame(oracle_mod, asset, CS.TORUS, CS.cam13(R, "offaxis"), 96, 54, 2, DEPTH)
    assert (LS.bits(a0) == LS.bits(want[0])).all() and (b0 == want[1]).all()
