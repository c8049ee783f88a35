"""The material classes of pipeline 4 on the CPU: tests/cpu_emul/matclass_main.cpp -- a stand-alone program over the C ABI, linked against the
product's own sources on the HIP stand-in under AddressSanitizer + UBSan, run directly (nothing preloaded) -- renders the cases of
tests/matclass_support.py with option "material_variants" 1.  Every dump must equal the oracle bit for bit (accumulator and ARGB), and the class
that ran is asserted: FLAT / FLAT_TEX for the flat scenes (no silent fallback to the general kernels), GENERAL for everything else.  The job
list is dealt out to several processes of the program that run side by side, each with its own context and output directory."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ASSETS, ROOT, asset

import raytracerwin_amd as R
import camera_support as CS
import matclass_support as MC
from oracle import oracle as _O  # (material node arrays only)


def job_line(out, c, second=None):
    name, mesh, tree, pose, w, h, n_passes, ns, depth, options, _ = c

    def nodes_file(nm, tr):
        if tr is None:
            return "-"
        path = out / (nm + ".nodes")
        _O.materials(tr).tofile(path)
        return str(path)
    eye, target, up, vfov = CS.POSES[pose] if pose else ((0.0, 0.0, 0.0),) * 3 + (0.0,)
    opts = dict(MC.OPTION_DEFAULTS, **options)
    return " ".join([name, mesh, nodes_file(name, tree), nodes_file(second[0], second[2]) if second else "-", "1", str(opts["split_paths"]), str(opts["primary_passes"]),
                     "1" if pose else "0"] + [repr(float(v)) for v in eye + target + up] + [repr(float(vfov))] + [str(v) for v in (w, h, n_passes, ns, depth)])


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    here = os.path.join(ROOT, "tests", "cpu_emul")
    subprocess.check_call(["make", "-C", here, "-f", "matclass.mk", "-j4"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    out = tmp_path_factory.mktemp("matclass_emul")
    lines = [job_line(out, c) for c in MC.CASES] + [job_line(out, MC.RECOMMIT, MC.RECOMMIT_SECOND)]
    frames = len(lines) + 1
    # the program carries the sanitizers' runtime itself (matclass.mk links it statically): the inherited environment, plus their options
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    n_procs = max(1, min(8, len(os.sched_getaffinity(0)), len(lines)))
    procs = []
    for k in range(n_procs):
        share = lines[k::n_procs]
        part = out / ("part%d" % k)
        part.mkdir()
        (part / "jobs.txt").write_text("\n".join(share) + "\n")
        log = (open(part / "stdout.txt", "w"), open(part / "stderr.txt", "w"))
        procs.append((subprocess.Popen([os.path.join(here, "_build", "matclass_main"), ASSETS, str(part), str(part / "jobs.txt")], stdout=log[0], stderr=log[1], env=env),
                      part, log))
    report = {}
    done = 0
    try:
        for proc, part, log in procs:
            rc = proc.wait(timeout=1800)
            for f in log:
                f.close()
            stdout, stderr = (part / "stdout.txt").read_text(), (part / "stderr.txt").read_text()
            assert rc == 0 and "matclass_main ok: " in stdout, (stdout[-1500:], stderr[-3000:])
            assert "runtime error" not in stderr and "AddressSanitizer" not in stderr, stderr[-3000:]
            done += int(stdout.split("matclass_main ok: ")[1].split()[0])
            for ln in (part / "report.txt").read_text().splitlines():
                report[ln.split()[0]] = (part, [int(v) for v in ln.split()[1:]])
    finally:
        for proc, *_ in procs:
            if proc.poll() is None:
                proc.kill()
    assert done == frames and len(report) == frames
    return report


def check(dumps, oracle_mod, c):
    part, (ran, cls) = dumps[c[0]]
    assert ran == 4, ran                                    # pipeline 4 ran
    assert cls == c[10], (cls, c[10])                       # ... with the kernels of the case's class: no silent fallback, and no flat kernel where it has no business
    want = MC.oracle_frame(oracle_mod, R, asset, c)
    accum, argb = np.fromfile(part / (c[0] + ".accum"), np.float32).reshape(-1, 4), np.fromfile(part / (c[0] + ".argb"), np.uint32)
    assert (MC.bits(accum) == MC.bits(want[0])).all() and (argb == want[1]).all()


@pytest.mark.parametrize("case", MC.FLAT_CASES, ids=MC.case_id)
def test_emulated_flat_scene_runs_its_class_and_equals_the_oracle(dumps, oracle_mod, case):
    check(dumps, oracle_mod, case)


@pytest.mark.parametrize("case", MC.FALLBACK_CASES, ids=MC.case_id)
def test_emulated_other_scene_stays_general_and_equals_the_oracle(dumps, oracle_mod, case):
    check(dumps, oracle_mod, case)


def test_emulated_class_follows_the_commit(dumps, oracle_mod):
    """a Diffuse scene rendered (FLAT), the committed scene refusing another material and another commit (the program stops otherwise), then the same
    mesh committed under the Blend in the same context and rendered into the same framebuffer: GENERAL, and both frames the oracle's"""
    check(dumps, oracle_mod, MC.RECOMMIT)
    check(dumps, oracle_mod, MC.RECOMMIT_SECOND)
