"""The camera through every touched kernel on the CPU: tests/cpu_emul/camera_main.cpp -- a stand-alone program over the C ABI, linked against
the product's own sources on the HIP stand-in under AddressSanitizer + UBSan, run directly (nothing preloaded) -- renders camera frames
at 96x54 through the pipelines 4, 3 and 0; its dumps must equal the oracle (tests/camera_support.py) bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ASSETS, ROOT, asset

import raytracerwin_amd as R
import camera_support as CS

W, H, DEPTH = 96, 54, 3
# (pose, pipeline, device_build, traversal, n_passes, sub_samples)
RUNS = [(4, 1, 1, 2, 2), (3, 0, 1, 1, 2), (0, 0, 1, 1, 2)]
JOBS = [(sc, pose) + run for sc in ("torus", "mixed") for pose in ("offaxis", "below", "inside", "away", "narrow", "wide") for run in RUNS]
JOBS += [("torus", "default", 4, 1, 1, 1, 4), ("torus", "offaxis", 4, 0, 1, 5, 1), ("torus", "offaxis", 0, 0, 0, 1, 1), ("mixed", "below", 4, 0, 1, 3, 1)]


def job_name(j):
    return "%s_%s_p%d_b%d_t%d_k%d_s%d" % j


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    here = os.path.join(ROOT, "tests", "cpu_emul")
    subprocess.check_call(["make", "-C", here, "-f", "camera.mk", "-j4"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    out = tmp_path_factory.mktemp("camera_emul")
    lines = []
    for j in JOBS:
        sc, pose, pipeline, dev, trav, npass, ns = j
        eye, target, up, vfov = CS.POSES[pose] if pose != "default" else ((0, 0, 7), (0, 0, 6), (0, 1, 0), -1.0)
        lines.append(" ".join([job_name(j), sc] + [repr(float(v)) for v in eye + target + up] + [repr(float(vfov))] +
                              [str(v) for v in (pipeline, dev, trav, W, H, npass, ns, DEPTH)]))
    jobs = out / "jobs.txt"
    jobs.write_text("\n".join(lines) + "\n")
    # the program carries the sanitizers' runtime itself (camera.mk links it statically): the inherited environment, plus their options
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(here, "_build", "camera_main"), ASSETS, str(out), str(jobs)], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0 and ("camera_main ok: %d frames" % len(JOBS)) in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    report = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in (out / "report.txt").read_text().splitlines()}
    return out, report


@pytest.mark.parametrize("job", JOBS, ids=job_name)
def test_emulated_camera_frame_equals_the_oracle(dumps, oracle_mod, job):
    out, report = dumps
    sc, pose, pipeline, dev, trav, npass, ns = job
    name = job_name(job)
    cam = np.fromfile(out / (name + ".cam"), np.float32)
    assert (CS.bits(cam) == CS.bits(CS.cam13(R, pose))).all()
    ran, has_bins, entries = report[name]
    assert ran == (pipeline if trav else 0), (ran, pipeline)
    if pose == "offaxis":
        assert has_bins == 1 and entries > 0
    if pose == "inside":
        assert has_bins == 0
    if pose == "away":
        assert has_bins == 1 and entries == 0          # every tile of the one-mesh scene is sky-only
    want = CS.oracle_frame(oracle_mod, asset, CS.SCENES[sc], cam, W, H, ns, DEPTH, n_passes=npass)
    accum = np.fromfile(out / (name + ".accum"), np.float32).reshape(-1, 4)
    argb = np.fromfile(out / (name + ".argb"), np.uint32)
    assert (CS.bits(accum) == CS.bits(want[0])).all() and (argb == want[1]).all()
