"""Per-pixel pass budgets through the kernels' BUDGET instantiations and rtw_budget_kernels.h on the CPU: tests/cpu_emul/budget_main.cpp -- a stand-alone
program over the C ABI, linked against the product's own sources on the HIP stand-in under AddressSanitizer + UBSan, run directly (nothing preloaded).
A 40 x 21 frame that holds two passes, 5 budgeted passes against the six uniform snapshots, bit for bit at every pixel, on TorusKnot (one group, groups of
two, a split group) and on the multi-shape scene; rtw_sample_budget at radius 2 against the float32 formula, integer for integer."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, ASSETS

import scenes as SC

W, H, N = 40, 21, 5
f32 = np.float32
TORUS = [("mesh", "TorusKnot", SC.diffuse((1, 1, 1)))]
# name, scene, sub-samples, group_max, split_paths, split_min (of the budgeted call)
JOBS = [("torus", TORUS, 2, 256, 400000, 8), ("torus_groups", TORUS, 1, 2, 400000, 8), ("torus_split", TORUS, 2, 256, 1, 4), ("multi", SC.default_scene(False), 1, 2, 400000, 8)]


def budget_pattern():
    py, px = np.mgrid[0:H, 0:W]
    b = np.array([-2, 0, 1, 2, 3, 4, 5, 6, 40], np.int32)[(7 * px + 3 * py) % 9]
    b[8:12, 16:32] = 0          # the frame's centre: on the mesh
    b[0:4, 0:16] = 0            # a corner: sky
    b[12:16, 16:32] = N
    return b


def sample_inputs():
    rng = np.random.default_rng(11)
    count = rng.integers(4, 30, (H, W)).astype(np.int32)
    count[:, 0], count[:, W - 1] = 3, 4           # below and at min_history
    mu = np.empty((H, W, 2), f32)
    mu[..., 0] = f32(0.5) + f32(0.5) * rng.random((H, W), dtype=f32)
    mu[..., 1] = mu[..., 0] * mu[..., 0] + rng.random((H, W), dtype=f32) ** 2 * (np.arange(W) / W).astype(f32)       # the noise grows from left to right
    mu[3, :, 1] -= f32(0.02)
    mu[5, :, 0] = 0
    mu[7, ::2, 0], mu[7, 1::2, 1], mu[9, ::2, :] = np.nan, np.inf, -np.inf
    return count, mu


def sample_reference(count, mu, tolerance, min_history, min_passes, max_passes, r):
    """include/rtwin.h's formula in float32, every operation rounded on its own"""
    mu1, mu2 = mu[..., 0], mu[..., 1]
    with np.errstate(all="ignore"):
        d = f32(tolerance) * (mu1 + f32(1e-3))
        x = np.fmax(mu2 - mu1 * mu1, f32(0)) / (d * d) - count.astype(f32)
        b0 = np.where(~(x < f32(max_passes)), max_passes, np.where(x <= f32(min_passes), min_passes, np.ceil(np.where(np.isfinite(x), x, 0)))).astype(np.int32)
    pad = np.zeros((H + 2 * r, W + 2 * r), np.int32)
    pad[r:r + H, r:r + W] = np.where(count < min_history, max_passes, b0)
    return np.max([pad[dy:dy + H, dx:dx + W] for dy in range(2 * r + 1) for dx in range(2 * r + 1)], axis=0)


@pytest.fixture(scope="module")
def dumps(tmp_path_factory, oracle_mod):
    here = os.path.join(ROOT, "tests", "cpu_emul")
    subprocess.check_call(["make", "-C", here, "-f", "budget.mk", "-j4"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    out = tmp_path_factory.mktemp("budget_emul")
    budget_pattern().tofile(out / "budget.i32")
    count, mu = sample_inputs()
    accum = np.zeros((H, W, 4), f32)
    accum[..., 3] = count.view(f32)
    accum.tofile(out / "sb_accum.f32")
    mu.tofile(out / "sb_mu.f32")
    with open(out / "jobs.txt", "w") as jobs:
        for name, shapes, ns, group_max, split_paths, split_min in JOBS:
            with open(out / (name + ".scene"), "w") as f:
                for i, sh in enumerate(shapes):
                    nodes = out / ("%s_%d.nodes" % (name, i))
                    oracle_mod.materials(sh[-1]).tofile(nodes)
                    f.write(" ".join([sh[0]] + [str(v) for part in sh[1:-1] for v in (part if isinstance(part, tuple) else (part,))] + [str(nodes)]) + "\n")
            jobs.write("%s %s %d %d %d %d\n" % (name, out / (name + ".scene"), ns, group_max, split_paths, split_min))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(here, "_build", "budget_main"), ASSETS, str(out)], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0 and "budget_main ok: %d jobs" % len(JOBS) in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    return out


@pytest.mark.parametrize("name", [j[0] for j in JOBS])
def test_emulated_budgeted_passes_equal_the_uniform_snapshots(dumps, name):
    load = lambda tag: (np.fromfile(dumps / (tag + ".accum"), np.uint32).reshape(-1, 4), np.fromfile(dumps / (tag + ".argb"), np.uint32))  # noqa: E731
    snaps = [load("%s_k%d" % (name, k)) for k in range(N + 1)]
    e = np.clip(budget_pattern(), 0, N).ravel()
    accum, argb = load(name)
    for j, got in enumerate((accum, argb)):
        want = np.stack([s[j] for s in snaps])[e, np.arange(H * W)]
        assert (got == want).all(), (j, np.flatnonzero((got != want).reshape(H * W, -1).any(axis=1))[:8])
    assert (snaps[N][0] != snaps[0][0]).any() and (accum != snaps[N][0]).any()


def test_emulated_sample_budget_equals_the_formula(dumps):
    count, mu = sample_inputs()
    want = sample_reference(count, mu, 0.25, 4, 2, 64, 2)
    got = np.fromfile(dumps / "sb.i32", np.int32).reshape(H, W)
    assert (want == 2).any() and (want == 64).any() and np.unique(want).size > 8
    assert (got == want).all(), np.argwhere(got != want)[:8]
