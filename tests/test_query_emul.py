"""The device-buffer ray queries on the CPU: tests/cpu_emul/query_main.cpp -- a stand-alone program over the C ABI, linked against the
product's own sources on the HIP stand-in under AddressSanitizer + UBSan, run directly (nothing preloaded) -- runs
rtw_trace_closest_device / rtw_trace_occluded_device / rtw_trace_occluded over the reference's golden rays; its dumps must equal the
fixtures bit for bit, the two kernels ("query_kernel" 1 and 0) each other byte for byte, and the any-hit bytes `shape >= 0`."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ASSETS, GOLDEN, ROOT

import scenes as SC

NS = (1, 63, 64, 65, None)          # None: every ray of the job
BLOCKS = (0, 1, 3)                  # 1 and 3: few blocks, so the batch loop makes several trips and the partial last batch comes on a later one
KERNELS = (1, 0)


def scene_text(shapes):
    out = []
    for sh in shapes:
        if sh[0] == "mesh":
            out.append("mesh %s" % sh[1])
        else:
            nums = [v for part in sh[1:-1] for v in (part if isinstance(part, (tuple, list)) else (part,))]
            out.append(sh[0] + " " + " ".join(repr(float(np.float32(v))) for v in nums))
    return "\n".join(out) + "\n"


# rays a job keeps of its fixture, spread evenly over it.  The stand-in runs a few hundred rays a second, so two jobs -- unitychan (a tree larger
# than the staged part, textures) and the texel-inheritance scene (analytic shapes) -- are long enough for a second trip of a wave through the batch
# loop (1100 rays = 18 batches on the 16 waves of ONE block, the last batch 12 rays, on a second trip); the GPU suite runs the full fixtures.
KEEP = {"torus_p0": 130, "torus_p1": 130, "unity": 1100, "quirk": 1100, "default_nofuzz": 130, "edges": 260}


def spread(idx, count):
    return idx[np.linspace(0, len(idx) - 1, count).astype(np.int64)]


def base_jobs():
    """name -> (scene text, fixture file, rays kept, prune)"""
    torus = np.load(os.path.join(GOLDEN, "closest_TorusKnot.npz"))
    unity = np.load(os.path.join(GOLDEN, "closest_unitychan.npz"))
    first400 = np.flatnonzero(~np.isnan(unity["rays"]).any(axis=1))       # (every ray without a NaN: 1100 of them are kept)
    jobs = {
        "torus_p0": ("mesh TorusKnot\n", torus, spread(np.arange(len(torus["rays"])), KEEP["torus_p0"]), 0),
        "torus_p1": ("mesh TorusKnot\n", torus, spread(np.arange(len(torus["rays"])), KEEP["torus_p1"]), 1),
        "unity": ("mesh unitychan\n", unity, spread(first400, KEEP["unity"]), 1),       # a tree larger than the staged part, with textures
    }
    for tag in ("quirk", "default_nofuzz"):
        g = np.load(os.path.join(GOLDEN, "sceneclosest_%s.npz" % tag))
        jobs[tag] = (scene_text(SC.SCENES[tag]()), g, spread(np.arange(len(g["rays"])), KEEP[tag]), 1)
    # the rays aimed at the analytic shapes' edges (tests/golden/make_golden.py:make_edge_rays): every family's share of the 260, at least 4 of each,
    # spread evenly over the family (so over its shapes).  Rays whose reference record holds a NaN (a NaN's sign and payload are not specified, and
    # the comparison below is on bits) stay with tests/test_edges_cpu.py and the GPU suite, which compare them by the NaN rule.
    g = np.load(os.path.join(GOLDEN, "sceneclosest_edges.npz"))
    usable = ~((g["shape"] >= 0) & np.isnan(g["hit"]).any(axis=1))
    keep = []
    for f in np.unique(g["family"]):
        idx = np.flatnonzero((g["family"] == f) & usable)
        keep.append(spread(idx, min(len(idx), max(4, round(KEEP["edges"] * len(idx) / len(usable))))))
    jobs["edges"] = (scene_text(SC.SCENES["edges"]()), g, np.unique(np.concatenate(keep)), 1)
    return jobs


def runs_of(base):
    r = [(base, n, qb, qk, 0) for n in NS for qb in BLOCKS for qk in KERNELS]
    return r + [(base, None, 0, 1, 1), (base, None, 3, 1, 2), (base, None, 1, 1, 3)]        # tri NULL; only shape; shape and tri without hits


BASES = ("torus_p0", "torus_p1", "unity", "quirk", "default_nofuzz", "edges")
RUNS = [r for b in BASES for r in runs_of(b)]


def run_name(r):
    return "%s_n%s_b%d_k%d_m%d" % (r[0], "all" if r[1] is None else r[1], r[2], r[3], r[4])


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    here = os.path.join(ROOT, "tests", "cpu_emul")
    subprocess.check_call(["make", "-C", here, "-f", "query.mk", "-j4"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    out = tmp_path_factory.mktemp("query_emul")
    jobs = base_jobs()
    lines = []
    for name, (text, g, keep, prune) in jobs.items():
        (out / (name + ".scene")).write_text(text)
        np.ascontiguousarray(g["rays"][keep], np.float32).tofile(out / (name + ".rays"))
    for r in RUNS:
        base, n, qb, qk, mode = r
        total = len(jobs[base][2])
        lines.append("%s %s %s %d %d %d %d %d" % (run_name(r), out / (base + ".scene"), out / (base + ".rays"), total if n is None else n, jobs[base][3], qk, qb, mode))
    (out / "jobs.txt").write_text("\n".join(lines) + "\n")
    # the program carries the sanitizers' runtime itself (query.mk links it statically): the inherited environment, plus their options
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(here, "_build", "query_main"), ASSETS, str(out), str(out / "jobs.txt")], capture_output=True, text=True, env=env, timeout=TIMEOUT)
    assert r.returncode == 0 and ("query_main ok: %d jobs" % len(RUNS)) in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    report = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in (out / "report.txt").read_text().splitlines()}
    return out, report, jobs


TIMEOUT = 1226      # twice the program's measured run on the CPU (600 s with the build, beside other work on the machine), plus twice the edges job's
                    # (its 33 runs alone: 13 s; the whole module with it, the program already built: 517 s)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("run", RUNS, ids=run_name)
def test_emulated_query_equals_the_fixture(dumps, run):
    out, report, jobs = dumps
    base, n, qb, qk, mode = run
    _, g, keep, _ = jobs[base]
    n = len(keep) if n is None else n
    keep = keep[:n]
    name = run_name(run)
    rays_c, boxes_c, tris_c, hits_c, rays_a, boxes_a, tris_a, guards, host_same = report[name]
    assert guards == 1, "a guard area beside an output buffer was written"
    assert host_same == 1, "rtw_trace_occluded (host arrays) differs from rtw_trace_occluded_device"
    shape = np.fromfile(out / (name + ".shape"), np.int32)
    want = g["shape"][keep]
    assert len(shape) == n and (shape == want).all()
    hit = want >= 0
    occ = np.fromfile(out / (name + ".occ"), np.uint8)
    assert (occ == hit.astype(np.uint8)).all()
    if mode <= 1:
        hits = np.fromfile(out / (name + ".hits"), np.float32).reshape(-1, 11)
        assert (bits(hits[hit]) == bits(g["hit"][keep][hit])).all()
    if mode in (0, 3) and "tri" in g.files:
        tri = np.fromfile(out / (name + ".tri"), np.int32)
        assert (tri[hit] == g["tri"][keep][hit]).all()
    assert rays_c == n and rays_a == n
    if qk == 1:
        assert boxes_a + tris_a <= boxes_c + tris_c         # a lane of the any-hit query stops at its first accepted test
        # shaded_hits counts the mesh finishes (as in the render kernels): every hit of a one-mesh scene, none when no record is asked for
        if mode >= 2:
            assert hits_c == 0
        elif base in ("torus_p0", "torus_p1", "unity"):
            assert hits_c == int(hit.sum())
        else:
            assert hits_c <= int(hit.sum())


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("qb", BLOCKS)
def test_emulated_query_kernels_agree_byte_for_byte(dumps, base, n, qb):
    """ "query_kernel" 1 (the ray-per-lane query kernel) and 0 (closest_kernel on the same buffers): every byte of every output, misses included"""
    out, _, _ = dumps
    a, b = run_name((base, n, qb, 1, 0)), run_name((base, n, qb, 0, 0))
    for ext in (".hits", ".shape", ".tri", ".occ"):
        assert (out / (a + ext)).read_bytes() == (out / (b + ext)).read_bytes(), ext
