"""The material trees of tests/material_support.py through every render kernel on the CPU: tests/cpu_emul/material_main.cpp -- a stand-alone
program over the C ABI, linked against the product's own sources on the HIP stand-in under AddressSanitizer + UBSan, run directly (nothing
preloaded) -- renders every tree at 32 x 18, 2 sub-samples, depth 5 through pipelines 0, 3 and 4 (and the depth-16 tree at 1 sub-sample); its
dumps must equal the oracle bit for bit (a NaN equals a NaN).  A frame costs the emulation some seconds, so the job list is dealt out to
several processes of the program that run side by side, each with its own context and output directory.  One job also offers every tree
rtw_scene_set_material must refuse, and asks for a bounce depth of 17: the program checks the return codes, and its frame must still be that
of the material set before."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ASSETS, ROOT, asset

import material_support as MS
from material_support import same
from oracle import oracle as _O  # (material node arrays only)

W, H, NS, DEPTH = 32, 18, 2, 5
PIPELINES = (4, 3, 0)
# (name, tree, pipeline, sub_samples, depth, preview)
JOBS = [(n, n, pl, NS, DEPTH, 0) for n in MS.ALL_TREES for pl in PIPELINES]
JOBS += [("bf_nan", "bf_nan", 4, NS, DEPTH, 1)]                              # PreviewColor: a Blend draws there too
JOBS += [("depth16", None, pl, 1, MS.MAX_BOUNCE, 0) for pl in PIPELINES]
REFUSALS = ("refusals", None, 4, NS, DEPTH, 0)


def job_name(j):
    return "%s_p%d_s%d_d%d_v%d" % ((j[0],) + j[2:])


def tree_of(j):
    return MS.DEPTH16_TREE if j[0] == "depth16" else MS.PREVIOUS if j[0] == "refusals" else MS.TREES[j[1]][0]


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    here = os.path.join(ROOT, "tests", "cpu_emul")
    subprocess.check_call(["make", "-C", here, "-f", "material.mk", "-j4"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    out = tmp_path_factory.mktemp("material_emul")
    bad = out / "bad.bin"
    with open(bad, "wb") as f:
        for name, (nodes, err) in sorted(MS.INVALID.items()):
            arr = _O.materials(nodes) if nodes else np.zeros(1, _O.MATERIAL_DTYPE)
            f.write(np.array([len(nodes), err], np.int32).tobytes() + arr.tobytes())
    lines = []
    for j in JOBS + [REFUSALS]:
        nodes = out / (job_name(j) + ".nodes")
        _O.materials(tree_of(j)).tofile(nodes)
        lines.append(" ".join([job_name(j), str(nodes)] + [str(v) for v in (j[2], W, H, j[3], j[4], j[5], 1)] + [str(bad) if j is REFUSALS else "-"]))
    # the program carries the sanitizers' runtime itself (material.mk links it statically): the inherited environment, plus their options
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    n_procs = max(1, min(8, len(os.sched_getaffinity(0))))
    procs = []
    for k in range(n_procs):
        share = lines[k::n_procs]
        part = out / ("part%d" % k)
        part.mkdir()
        (part / "jobs.txt").write_text("\n".join(share) + "\n")
        log = (open(part / "stdout.txt", "w"), open(part / "stderr.txt", "w"))
        procs.append((subprocess.Popen([os.path.join(here, "_build", "material_main"), ASSETS, str(part), str(part / "jobs.txt")], stdout=log[0], stderr=log[1], env=env),
                      part, len(share), log))
    report = {}
    try:
        for proc, part, n, log in procs:
            rc = proc.wait(timeout=1800)
            for f in log:
                f.close()
            stdout, stderr = (part / "stdout.txt").read_text(), (part / "stderr.txt").read_text()
            assert rc == 0 and ("material_main ok: %d frames" % n) in stdout, (stdout[-1500:], stderr[-3000:])
            assert "runtime error" not in stderr and "AddressSanitizer" not in stderr, stderr[-3000:]
            for ln in (part / "report.txt").read_text().splitlines():
                report[ln.split()[0]] = (part, [int(v) for v in ln.split()[1:]])
    finally:
        for proc, *_ in procs:
            if proc.poll() is None:
                proc.kill()
    assert len(report) == len(JOBS) + 1
    return report


def check(dumps, oracle_mod, j):
    name = job_name(j)
    out, (ran, offered) = dumps[name]
    assert ran == j[2], (ran, j[2])                         # the pipeline asked for ran (32 x 18 tiles for pipeline 3): no fallback
    fuzzy = j[1] is not None and not MS.TREES[j[1]][1]
    want = MS.oracle_frame(oracle_mod, MS.oracle_scene(oracle_mod, asset, tree_of(j), fuzzy=fuzzy), W, H, j[3], j[4], bool(j[5]))
    accum, argb = np.fromfile(out / (name + ".accum"), np.float32).reshape(-1, 4), np.fromfile(out / (name + ".argb"), np.uint32)
    assert (argb == want[1]).all()
    if not j[5]:
        assert same(accum, want[0])
    return offered


@pytest.mark.parametrize("job", JOBS, ids=job_name)
def test_emulated_frame_equals_the_oracle(dumps, oracle_mod, job):
    check(dumps, oracle_mod, job)


def test_emulated_refusals_leave_the_previous_material_in_force(dumps, oracle_mod):
    """every tree of MS.INVALID returned its stated error (the program stops otherwise), max_bounce 17 was refused by rtw_render_passes and
    rtw_ray_trace and 16 accepted, the scene then committed, and its frame is the frame of the material set before the refusals"""
    assert check(dumps, oracle_mod, REFUSALS) == len(MS.INVALID)
