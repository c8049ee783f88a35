"""First-hit feature buffers through both feature kernels on the CPU: tests/cpu_emul/features_main.cpp -- a stand-alone program over the C ABI, linked
against the product's own sources on the HIP stand-in under AddressSanitizer + UBSan, run directly (nothing preloaded) -- renders the buffers of a
dozen small frames; every dump must equal the model of tests/features_support.py (the oracle behind the ray models) bit for bit.  The program
also tries every call rtw_render_features must refuse and checks that feature calls leave the work counters alone."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ASSETS, ROOT, asset

import raytracerwin_amd as R
import camera_support as CS
import features_support as FS
import lens_support as LS

RADIUS = 0.2
# (scene, pose, lens radius, traversal, width, height, first_pass, n_passes, sub_samples, task_rows, rank, world, calls)
JOBS = [
    ("torus", None, 0.0, 1, 96, 54, 0, 1, 2, 10, 0, 1, 1),          # no camera set: the fixed-pose instantiations, bins
    ("torus", "offaxis", 0.0, 1, 96, 54, 0, 1, 4, 10, 0, 1, 1),     # bins under a general pose; four sub-samples in one walk
    ("torus", "inside", 0.0, 1, 96, 54, 0, 1, 2, 10, 0, 1, 1),      # no bins: the packet walk
    ("mixed", None, 0.0, 1, 96, 54, 0, 1, 2, 10, 0, 1, 1),
    ("mixed", "offaxis", 0.0, 1, 96, 54, 0, 1, 2, 10, 0, 1, 1),     # analytic shapes around a mesh with bins: the per-lane bins loop
    ("mixed", "inside", 0.0, 1, 96, 54, 0, 1, 1, 10, 0, 1, 1),
    ("mixed", "offaxis", RADIUS, 1, 96, 54, 0, 1, 2, 10, 0, 1, 1),  # a lens
    ("torus", "offaxis", 0.0, 1, 96, 54, 0, 5, 1, 10, 0, 1, 1),     # five passes in one call: four ray sets and a fifth that starts a new batch
    ("torus", "offaxis", 0.0, 1, 96, 54, 3, 2, 2, 10, 0, 1, 2),     # two calls of one pass, from pass 3 on
    ("torus", "offaxis", 0.0, 1, 50, 37, 0, 1, 2, 10, 0, 1, 1),     # a frame that does not tile into whole 64-pixel tiles
    ("mixed", "offaxis", 0.0, 1, 50, 37, 0, 2, 2, 10, 1, 2, 1),     # world 2, rank 1
    ("torus", "offaxis", 0.0, 1, 96, 54, 0, 1, 2, 6, 0, 2, 1),      # world 2, tasks of 6 rows: 32 x 2-pixel tiles
    ("torus", "offaxis", 0.0, 0, 96, 54, 0, 1, 2, 10, 0, 1, 1),     # traversal 0: the same buffers
]


def job_name(j):
    return "%s_%s_a%g_t%d_%dx%d_p%d_k%d_s%d_r%d_%dof%d_c%d" % j


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    here = os.path.join(ROOT, "tests", "cpu_emul")
    subprocess.check_call(["make", "-C", here, "-f", "features.mk", "-j4"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    out = tmp_path_factory.mktemp("features_emul")
    lines = []
    for j in JOBS:
        sc, pose, radius, traversal, W, H, first, npass, ns, rows, rank, world, calls = j
        eye, target, up, vfov = CS.POSES[pose or "offaxis"]
        lines.append(" ".join([job_name(j), sc, "0" if pose is None else "1"] + [repr(float(v)) for v in eye + target + up] +
                              [repr(float(vfov)), repr(float(radius)), repr(LS.target_distance(CS.POSES[pose or "offaxis"]))] +
                              [str(v) for v in (traversal, W, H, first, npass, ns, rows, rank, world, calls)]))
    jobs = out / "jobs.txt"
    jobs.write_text("\n".join(lines) + "\n")
    # the program carries the sanitizers' runtime itself (features.mk links it statically): the inherited environment, plus their options
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(here, "_build", "features_main"), ASSETS, str(out), str(jobs)], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0 and ("features_main ok: %d frames, refusals checked" % len(JOBS)) in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    return out


@pytest.mark.parametrize("job", JOBS, ids=job_name)
def test_emulated_feature_buffers_equal_the_model(dumps, oracle_mod, job):
    sc, pose, radius, traversal, W, H, first, npass, ns, rows, rank, world, calls = job
    name = job_name(job)
    got = (np.fromfile(dumps / (name + ".geom"), np.float32).reshape(-1, 4), np.fromfile(dumps / (name + ".albedo"), np.float32).reshape(-1, 4),
           np.fromfile(dumps / (name + ".ids"), np.int32).reshape(-1, 2))
    lens = (np.float32(radius), np.float32(LS.target_distance(CS.POSES[pose]))) if radius > 0 else None
    want = FS.model(oracle_mod, asset, CS.SCENES[sc], CS.cam13(R, pose), lens, W, H, ns, first_pass=first, n_passes=npass, task_rows=rows, rank=rank, world=world)
    assert FS.same(got, want), FS.first_difference(got, want)
    if world > 1:       # the other rank's pixels stay as rtw_features_clear left them
        other = np.setdiff1d(np.arange(W * H), FS.share_pixels(W, H, rows, rank, world))
        assert len(other) and (got[0][other] == 0).all() and (got[1][other] == 0).all() and (got[2][other] == -1).all()
