"""Edge cases of the leaf operations every pipeline shares, on the CPU: the oracle against fixtures the REAL reference wrote for rays aimed at the
analytic shapes' tangents, surfaces, segment ends, seams and axes (sceneclosest_edges.npz) and for textures of awkward shapes
(tests/golden/oddtex/, texsample_oddtex_m{k}.npz) -- and the fixtures themselves: a fixture that stops probing anything fails here."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, asset

import scenes as SC
from tests.golden.make_golden import EDGE_FAMILIES, EDGE_ULP_FAMILIES, ODDTEX, ODDTEX_UV, make_edge_rays, oddtex_texels

ODDTEX_OBJ = os.path.join(GOLDEN, "oddtex", "oddtex.obj")
# shapes of scene "edges" that the reference reports for no ray of the fixture: a sphere of radius 0 (only a ray through the exact centre has a
# discriminant of 0, and float32 rounding leaves it below 0 for every ray drawn) and a plane whose normal is (0, 0, 0) (its denominator is 0)
NEVER_HIT = {1: "sphere of radius 0", 8: "plane with a zero normal"}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    """bit-identical, except that any NaN equals any NaN (payload/sign of a NaN is not specified)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.fixture(scope="module")
def edges():
    g = np.load(os.path.join(GOLDEN, "sceneclosest_edges.npz"))
    return {k: g[k] for k in g.files}


def test_edges_fixture_still_probes_every_shape_and_every_edge(edges):
    """In the reference's own output: every shape that can be hit at all is both hit and missed by the rays aimed at it; each family whose rays
    differ by a few ulps (tangent, segment end, parallel to a capsule's axis at its radius, seam, triangle vertex and edge) is decided both ways,
    20 % to 80 % hits of the shape aimed at; the shapes that can never be hit are exactly the ones listed."""
    scene = SC.SCENES["edges"]()
    rays, family, target, shape = edges["rays"], edges["family"], edges["target"], edges["shape"]
    assert rays.dtype == np.float32 and len(rays) <= 4000 and len(family) == len(target) == len(shape) == len(rays)
    assert sorted(set(family.tolist())) == list(range(len(EDGE_FAMILIES)))
    assert sorted(set(target.tolist())) == list(range(len(scene)))
    assert [sh[0] for sh in scene].index("mesh") not in (0, len(scene) - 1)
    own = shape == target
    for k, sh in enumerate(scene):
        aimed = target == k
        if k in NEVER_HIT:
            assert not (shape == k).any(), NEVER_HIT[k]
        else:
            assert own[aimed].any() and not own[aimed].all(), (k, sh[0])
    for name in EDGE_ULP_FAMILIES:
        m = family == EDGE_FAMILIES.index(name)
        share = own[m].mean()
        print("%s: %d rays, %.0f %% hit the shape aimed at" % (name, int(m.sum()), 100 * share))
        assert m.sum() >= 60 and 0.2 <= share <= 0.8, name
    near = (family == EDGE_FAMILIES.index("plane_near_parallel")) & (target == 7)       # |normal . direction| on either side of the test's 1e-6
    assert own[near].any() and not own[near].all()
    assert (shape == 4).any() and (shape == 6).any()        # the two coincident spheres: either may be reported, by the last bit of the second test
    odd = family == EDGE_FAMILIES.index("odd")
    assert {scene[k][0] for k in set(target[odd].tolist())} == {"sphere", "plane", "capsule", "triangle", "mesh"}
    assert np.isnan(rays[odd]).any() and np.isinf(rays[odd]).any() and (rays[odd][:, 6] <= 0).any() and (rays[odd][:, 3:6] == 0).all(axis=1).any()


def test_edge_rays_are_reproducible_from_their_seed(edges):
    rays, family, target = make_edge_rays(SC.SCENES["edges"](), np.random.default_rng(20261021))
    assert rays.tobytes() == edges["rays"].tobytes() and (family == edges["family"]).all() and (target == edges["target"]).all()


def test_oracle_equals_the_reference_on_the_edge_rays(oracle_mod, edges):
    """trace_closest of the oracle over the reference's records: the same shape for every ray, the same bits in every record of a hit (NaN == NaN:
    a huge sphere met by a 1e30 segment and a triangle met by a NaN ray are hits whose records hold NaN), family by family for the message."""
    s = oracle_mod.Scene().add_shapes(SC.SCENES["edges"](), lambda n: asset(n + ".obj"))
    hf, hs, _ = s.trace_closest(edges["rays"])
    for f, name in enumerate(EDGE_FAMILIES):
        m = edges["family"] == f
        assert (hs[m] == edges["shape"][m]).all(), name
        hit = m & (hs >= 0)
        assert same(hf[hit], edges["hit"][hit]), name
    assert (hs >= 0).sum() > 1000 and np.isnan(edges["hit"][hs >= 0]).any()


# ---- textures of awkward shapes ----
def test_oddtex_fixture_has_the_awkward_sizes_and_reaches_every_texel():
    from PIL import Image
    for k, (w, h, c) in enumerate(ODDTEX):
        im = Image.open(os.path.join(GOLDEN, "oddtex", "t%d.png" % k))
        assert im.size == (w, h) and im.mode == ("RGB", "RGBA")[c - 3]
        px = np.asarray(im)
        assert (px == oddtex_texels(k)).all()
        assert len(np.unique(px[:, :, :3].reshape(-1, 3), axis=0)) == w * h and (c == 3 or len(np.unique(px[:, :, 3])) == w * h)
        g = np.load(os.path.join(GOLDEN, "texsample_oddtex_m%d.npz" % k))
        uv = g["uv"]
        assert uv.dtype == np.float32 and uv.shape == (300, 2) and np.isfinite(uv).all()        # (a NaN or inf uv reads out of bounds in the reference)
        for n, col in ((w, 0), (h, 1)):         # every column and row, exactly and from either side
            for i in range(n if n > 1 else 0):
                at = np.float32(i) / np.float32(n - 1)
                for v in (at, np.nextafter(at, np.float32(-1)), np.nextafter(at, np.float32(2))):
                    assert (uv[:, col] == v).any(), (k, col, i)
        for v in (-1e-9, 1 - 2.0 ** -24, 8388607.5, 1e9, -1e9, -1.0, -3.0):
            assert (uv == np.float32(v)).any()
        assert (np.signbit(uv) & (uv == 0)).any()
    assert {(w == 1, h == 1) for w, h, _ in ODDTEX} == {(True, True), (True, False), (False, True), (False, False)}
    flat = np.array(ODDTEX_UV, np.float32)
    assert (flat == 0).any() and (flat == 1).any() and (flat < 0).any() and (flat > 1).any()


@pytest.mark.parametrize("k", range(len(ODDTEX)))
def test_oracle_texture_sample_equals_the_reference_on_awkward_sizes(oracle_mod, k):
    """RTexture::Sample through the reference's own PNG loader (every size loaded: 1 x 1, 1 x 9, 7 x 1, 5 x 3, 33 x 17; RGB and RGBA) against the
    oracle, which gets its texels from Pillow; and against the oracle handed the texel array itself."""
    g = np.load(os.path.join(GOLDEN, "texsample_oddtex_m%d.npz" % k))
    s = oracle_mod.Scene()
    sh = s.add_mesh_obj(ODDTEX_OBJ)
    assert (bits(s.texture_sample(sh, k, g["uv"])) == bits(g["rgba"])).all()
    fed = oracle_mod.Scene()
    sh = fed.add_mesh_obj(ODDTEX_OBJ, load_textures=False)
    fed.set_texture(sh, k, oddtex_texels(k))
    assert (bits(fed.texture_sample(sh, k, g["uv"])) == bits(g["rgba"])).all()
    assert len(np.unique(g["rgba"], axis=0)) >= min(ODDTEX[k][0] * ODDTEX[k][1], 40)
