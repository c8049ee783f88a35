"""The material tree at its edges and limits, without a GPU: (1) the oracle (oracle/rt_oracle.c) against the reference's own BounceViewRay /
PreviewColor on the trees of tests/material_support.py (tests/golden/matedge_*.npz), bit for bit (a NaN equals a NaN); (2) conditions which
show that those inputs reach the edges they are named after; (3) rtw_scene_set_material's validation on a host-only scene (the part that needs
a device -- the previous material stays in force, the scene still renders, the bounce limit -- is in tests/test_material_emul.py and
tests/test_material_gpu.py)."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, asset

import material_support as MS
import scenes as SC
from oracle import oracle as _O  # (material node arrays only)
from material_support import bits, same

W, H, NS, DEPTH = MS.FRAME


def golden(name):
    return np.load(os.path.join(GOLDEN, "matedge_%s.npz" % name))


@pytest.fixture(scope="module")
def shared_rays():
    return np.load(os.path.join(GOLDEN, "matedge_rays.npz"))


def frame(O, name, preview=False, depth=DEPTH):
    return MS.oracle_tree_frame(O, asset, name, W, H, NS, depth, preview)


# ---- 1. the oracle against the reference ------------------------------------------------------------------------------------------------------
def test_every_ref_tree_has_its_fixture_and_no_other_exists():
    have = sorted(f[8:-4] for f in os.listdir(GOLDEN) if f.startswith("matedge_") and f.endswith(".npz") and f != "matedge_rays.npz")
    assert have == MS.REF_TREES
    for name in MS.REF_TREES:
        g = golden(name)
        assert g["material"].tobytes() == _O.materials(MS.TREES[name][0]).tobytes(), name
        assert [int(v) for v in g["params"]] == [W, H, NS, DEPTH, 0, MS.SEED, 0, 1]
    assert [SC.matedge_scene()[k][-1] for k in range(3)] == [MS.TREES[n][0] for n in MS.MATEDGE_SCENE_TREES]


@pytest.mark.parametrize("name", MS.REF_TREES)
def test_oracle_equals_the_reference_on_the_tree(oracle_mod, shared_rays, name):
    """frame, preview frame and the ray_trace record of matedge_<name>.npz"""
    g = golden(name)
    accum, argb = frame(oracle_mod, name)
    assert same(accum, g["accum"]) and (argb == g["argb"]).all()
    assert (frame(oracle_mod, name, preview=True)[1] == g["preview_argb"]).all()
    depth, seed, RW, RH = [int(v) for v in shared_rays["params"]]
    rgb = MS.oracle_scene(oracle_mod, asset, g["material"]).ray_trace(shared_rays["rays"], shared_rays["keys"], depth, False, seed, RW, RH)
    assert same(rgb, g["rgb"])


# sceneframe_matedge_*.npz and frame_torus_*_d16.npz are picked up by tests/test_oracle_golden.py's lists; the scene is added to them here
@pytest.mark.parametrize("name", ["matedge_d5", "matedge_preview"])
def test_oracle_equals_the_reference_on_the_scene_file(oracle_mod, name):
    g = np.load(os.path.join(GOLDEN, "sceneframe_%s.npz" % name))
    Wd, Hd, ns, depth, preview, seed, pass0, npass = [int(v) for v in g["params"]]
    s = oracle_mod.Scene().add_shapes(SC.SCENES[str(g["scene"])](), lambda n: asset(n + ".obj"))
    accum, argb = MS.oracle_frame(oracle_mod, s, Wd, Hd, ns, depth, bool(preview), npass, seed)
    assert (argb == g["argb"]).all()
    if not preview:
        assert same(accum, g["accum"])
        hit = np.abs(accum[:, :3] - accum[0, :3]).max(axis=1) > 0
        assert hit.mean() > 0.5 and np.isfinite(accum[hit]).all()


# ---- 2. the inputs reach the edges ---------------------------------------------------------------------------------------------------------
def equal(O, a, b, preview=False):
    (aa, ab), (ba, bb) = frame(O, a, preview), frame(O, b, preview)
    return same(aa, ba) and (ab == bb).all()


def test_combine_operand_order_shows(oracle_mod):
    assert not equal(oracle_mod, "co_em_d", "co_d_em")
    # combine(Emissive, Diffuse): the ray that goes on is the incoming one, so a path that hits the mesh hits it at every level; the Diffuse
    # operand first (B before A) sends its own ray on
    a, b = frame(oracle_mod, "co_em_d", depth=DEPTH)[0], frame(oracle_mod, "co_em_d", depth=DEPTH - 1)[0]
    hit = mesh_pixels(oracle_mod)
    assert (bits(a[hit]) != bits(b[hit])).any(axis=1).mean() > 0.9


def test_blend_factor_clamp_and_nan(oracle_mod):
    O = oracle_mod
    for preview in (False, True):
        assert equal(O, "bf_m05", "bf_0", preview) and equal(O, "bf_15", "bf_1", preview)
        assert not equal(O, "bf_0", "bf_05", preview) and not equal(O, "bf_1", "bf_05", preview) and not equal(O, "bf_0", "bf_1", preview)
        assert equal(O, "bf_nan", "bf_1", preview)         # Random() > NaN is false: always B, as with factor 1
    g, g1 = golden("bf_nan"), golden("bf_1")               # and that is how the reference reads it
    assert same(g["accum"], g1["accum"]) and (g["argb"] == g1["argb"]).all() and (g["preview_argb"] == g1["preview_argb"]).all() and same(g["rgb"], g1["rgb"])


def test_checker_size_switch(oracle_mod):
    O = oracle_mod
    for preview in (False, True):
        for tag in ("below_eps", "1e_8", "1e_30", "0"):             # every size below FLT_EPSILON in magnitude counts as 1
            assert equal(O, "ck_" + tag, "ck_1", preview), tag
        for tag in ("eps", "m2", "1e30", "inf"):
            assert not equal(O, "ck_" + tag, "ck_1", preview), tag
    assert same(golden("ck_below_eps")["accum"], golden("ck_1")["accum"]) and not same(golden("ck_eps")["accum"], golden("ck_1")["accum"])


def test_albedo_channels_through_the_nonzero_test(oracle_mod):
    O = oracle_mod
    assert equal(O, "alb_negzero", "alb_zero")
    assert same(golden("alb_negzero")["accum"], golden("alb_zero")["accum"])           # the reference agrees
    assert equal(O, "alb_denorm", "alb_zero")                                          # |1e-40| < FLT_EPSILON: the path ends at the hit
    assert not equal(O, "alb_neg", "alb_zero") and not equal(O, "alb_3", "alb_zero")
    for name in ("alb_inf", "alb_nan"):
        a = frame(O, name)[0]
        assert (~np.isfinite(a)).any(), name                                          # the odd channel did reach a pixel


def test_fuzz_that_draws_nothing(oracle_mod):
    O = oracle_mod
    for pre in ("fz_", "co_fz_"):
        assert equal(O, pre + "m1", pre + "0")
        assert same(golden(pre + "m1")["accum"], golden(pre + "0")["accum"])
        for tag in ("1e_30", "1", "50"):
            assert not equal(O, pre + tag, pre + "0"), pre + tag
    # under the Combine the two draws of a positive fuzz move the sibling's pixels too: wherever the mesh is hit, not only in a few pixels
    a, b = frame(O, "co_fz_1e_30")[0], frame(O, "co_fz_0")[0]
    assert (bits(a) != bits(b)).any(axis=1)[mesh_pixels(O)].mean() > 0.5


_mesh_pixels = []


def mesh_pixels(O):
    """pixels of the 48 x 27 frame in which at least one camera ray hits the mesh (a bright Emissive at depth 1 marks them)"""
    if not _mesh_pixels:
        a, _ = MS.oracle_frame(O, MS.oracle_scene(O, asset, MS.emissive((7.0, 7.0, 7.0))), W, H, NS, 1)
        _mesh_pixels.append(a[:, 0] > 3.0)                  # one of two sub-samples is enough: 3.5 + half a sky
        assert 30 <= _mesh_pixels[0].sum()                 # the knot is small in this frame: some 40 pixels
    return _mesh_pixels[0]


def test_depth_16_reaches_the_last_level(oracle_mod):
    """frame_torus_combine_d16.npz: every path that hits the mesh carries all 16 levels (depth 15 differs in nearly each such pixel).  The mirror the
    issue names (frame_torus_mirror_d16.npz) does not get there: on this mesh no mirrored path of the frame survives 8 reflections, depth 16 and
    depth 8 give the same frame bit for bit -- recorded here, and the reason the second fixture exists."""
    O = oracle_mod
    d = MS.DEPTH16
    mirror = MS.oracle_scene(O, asset, d["material"])
    f = lambda s, depth, hist=None: MS.oracle_frame(O, s, d["W"], d["H"], d["ns"], depth, seed=d["seed"], history=hist)  # noqa: E731
    assert same(f(mirror, 16)[0], f(mirror, 8)[0]) and not same(f(mirror, 16)[0], f(mirror, 4)[0])
    s = MS.oracle_scene(O, asset, MS.DEPTH16_TREE)
    a16, a15 = f(s, 16)[0], f(s, 15)[0]
    g = np.load(os.path.join(GOLDEN, "frame_torus_combine_d16.npz"))
    assert same(a16, g["accum"]) and g["material"].tobytes() == _O.materials(MS.DEPTH16_TREE).tobytes()
    a1 = MS.oracle_frame(O, MS.oracle_scene(O, asset, MS.emissive((7.0, 7.0, 7.0))), d["W"], d["H"], d["ns"], 1, seed=d["seed"])[0]
    hit = a1[:, 0] > 6.0
    assert hit.sum() >= 20
    differs = (bits(a16) != bits(a15)).any(axis=1)                   # the 16th level's emission, through 15 attenuations, still moves the sum
    assert differs[hit].mean() > 0.9 and not differs[~hit].any()
    for tag in ("torus_combine_d16", "torus_mirror_d16"):           # most mesh pixels finite in the reference here too (the NaN rule hides nothing)
        assert np.isfinite(np.load(os.path.join(GOLDEN, "frame_%s.npz" % tag))["accum"][hit]).all(axis=1).mean() >= 0.5, tag


@pytest.mark.parametrize("name", MS.REF_TREES)
def test_most_mesh_pixels_are_finite_in_the_reference(oracle_mod, shared_rays, name):
    """otherwise NaN == NaN could hide a failure"""
    g = golden(name)
    hit = mesh_pixels(oracle_mod)
    assert np.isfinite(g["accum"][hit]).all(axis=1).mean() >= 0.5
    assert np.isfinite(g["rgb"]).all(axis=1).mean() >= 0.5


def test_the_random_family_is_valid_and_wide():
    fam = MS.random_family()
    assert len(fam) == 40 and [_O.materials(t).tobytes() for t in fam] == [_O.materials(t).tobytes() for t in MS.random_family()]
    nest = [MS.combine_nesting(t) for t in fam]
    assert all(n is not None and n <= 2 for n in nest) and all(1 <= len(t) <= MS.MAX_NODES for t in fam)
    assert nest.count(2) >= 10 and max(len(t) for t in fam) > 40
    assert all(not (t == SC.RF and p > 0) for tree in fam for t, _, p, _, _ in tree)          # fuzz-free: valid input for the reference too
    params = [p for tree in fam for t, _, p, _, _ in tree if t in (SC.BL, SC.DC)]
    assert any(np.isnan(p) for p in params) and any(p < 0 for p in params) and any(np.isinf(p) for p in params)
    for name in MS.ALL_TREES:
        assert MS.combine_nesting(MS.TREES[name][0]) in (0, 1, 2), name
    for name, (nodes, err) in MS.INVALID.items():
        ok = 1 <= len(nodes) <= MS.MAX_NODES and all(0 <= n[0] <= 6 for n in nodes) and MS.combine_nesting(nodes) is not None and MS.combine_nesting(nodes) <= 2
        assert not ok, name


# ---- 3. rtw_scene_set_material's validation, on a host-only scene -----------------------------------------------------------------------------
def _nodes(nodes):
    return _O.materials(nodes) if nodes else np.zeros(1, _O.MATERIAL_DTYPE)       # zero nodes: a valid pointer with a count of 0


def _host_scene():
    import raytracerwin_amd as R
    s = R.RayTracerScene(None)                                    # no context: parse, validate and build only
    s.AddShape(R.RSphere.Create((0.0, 0.0, 0.0), 1.0), R.material_nodes_from_array(_nodes(MS.PREVIOUS)))
    return R, s


@pytest.fixture(scope="module")
def host_scene():
    R, s = _host_scene()
    yield R, s
    s.close()


def set_material(R, s, nodes):
    arr = _nodes(nodes)
    return R.api.library().rtw_scene_set_material(s.h, 0, arr.ctypes.data_as(C.c_void_p), len(nodes))


@pytest.mark.parametrize("name", sorted(MS.INVALID))
def test_set_material_refuses(host_scene, name):
    R, s = host_scene
    nodes, err = MS.INVALID[name]
    assert set_material(R, s, nodes) == err
    said = R.api.library().rtw_last_error().decode()             # and says why
    assert ("node count" in said) if err == MS.ERR_LIMIT and len(nodes) not in range(1, MS.MAX_NODES + 1) else \
        ("nesting" in said) if err == MS.ERR_LIMIT else ("type" in said or "children" in said), said
    assert set_material(R, s, MS.PREVIOUS) == 0                   # the scene is still usable


def test_set_material_accepts_the_limits():
    R, s = _host_scene()
    assert set_material(R, s, MS.GARBAGE_LEAVES) == 0             # a leaf's child fields are never read
    assert set_material(R, s, MS.TREES["nodes64"][0]) == 0
    for name in MS.ALL_TREES:
        assert set_material(R, s, MS.TREES[name][0]) == 0, name
    for tree in MS.random_family():
        assert set_material(R, s, tree) == 0
    for name, (nodes, err) in MS.INVALID.items():
        assert set_material(R, s, nodes) == err
    s.commit()                                                    # after all the refusals the scene still commits
    assert set_material(R, s, MS.PREVIOUS) == -5                  # RTW_ERR_STATE: committed
    s.close()
