"""Shared by the material-class tests (data and the oracle's frames; no test in here).

A case: (name, mesh, tree, pose, width, height, n_passes, sub_samples, depth, options, class), tree None = the mesh gets no material, pose
None = no camera is ever set, options = context options of the case beside "material_variants", class = the material class pipeline 4 must
report for it with "material_variants" 1 (0 GENERAL, 1 FLAT, 2 FLAT_TEX; include/rtwin.h)."""
import numpy as np

import camera_support as CS
import scenes as SC

GENERAL, FLAT, FLAT_TEX = 0, 1, 2
SEED = 12345
W, H, NP, NS, DEPTH = 96, 54, 2, 2, 4
BLEND = SC.blend(SC.reflective((1, 1, 1), 0.2), SC.diffuse((1, 1, 1)), 0.5)              # bench.py's C3 material
FUZZY = SC.reflective((0.9, 0.9, 0.9), 0.2)
COMBINE = SC.combine(SC.diffuse((0.2, 0.8, 0.3)), SC.emissive((0.3, 0.1, 0.1)))
UNFUZZED = (SC.RF, SC.BL)     # trees with these nodes can draw a fuzzy direction: the oracle follows them in its double-precision mode

FLAT_CASES = [
    ("torus_diffuse", "TorusKnot", SC.diffuse(), None, W, H, NP, NS, DEPTH, {}, FLAT),
    ("torus_checker", "TorusKnot", SC.checker((0.9, 0.8, 0.7), 0.3), None, W, H, NP, NS, DEPTH, {}, FLAT),
    ("unitychan_diffuse", "unitychan", SC.diffuse(), None, W, H, NP, NS, DEPTH, {}, FLAT_TEX),       # its texels carry alpha: the transparent branch, the draw consumed or not
    ("torus_partial_tiles", "TorusKnot", SC.diffuse(), None, 50, 37, NP, NS, DEPTH, {}, FLAT),
    ("torus_8_passes_split", "TorusKnot", SC.diffuse(), None, W, H, 8, NS, DEPTH, {"split_paths": 0}, FLAT),     # a split group: two parts
    ("torus_5_passes_4_rays", "TorusKnot", SC.diffuse(), None, W, H, 5, NS, DEPTH, {"primary_passes": 4}, FLAT),  # one part; 2 passes x 2 sub-samples per lane of the primary kernel
    ("torus_depth1", "TorusKnot", SC.diffuse(), None, W, H, NP, NS, 1, {}, FLAT),                     # the first ...
    ("torus_depth16", "TorusKnot", SC.diffuse(), None, W, H, NP, NS, 16, {}, FLAT),                   # ... and the last level of the level store
    ("torus_offaxis", "TorusKnot", SC.diffuse(), "offaxis", W, H, NP, NS, DEPTH, {}, FLAT),           # the general camera's instantiation
]
FALLBACK_CASES = [
    ("monkey_blend", "BlenderMonkey", BLEND, None, W, H, NP, NS, DEPTH, {}, GENERAL),
    ("torus_fuzzy", "TorusKnot", FUZZY, None, W, H, NP, NS, DEPTH, {}, GENERAL),
    ("torus_combine", "TorusKnot", COMBINE, None, W, H, NP, NS, DEPTH, {}, GENERAL),
    ("torus_no_material", "TorusKnot", None, None, W, H, NP, NS, DEPTH, {}, GENERAL),
]
CASES = FLAT_CASES + FALLBACK_CASES
# the class follows the commit: a Diffuse scene rendered, then the same mesh committed under the Blend in the same context and rendered
RECOMMIT = ("torus_recommit", "TorusKnot", SC.diffuse(), None, W, H, NP, NS, DEPTH, {}, FLAT)
RECOMMIT_SECOND = ("torus_recommit_re", "TorusKnot", BLEND, None, W, H, NP, NS, DEPTH, {}, GENERAL)
OPTION_DEFAULTS = {"split_paths": 400000, "primary_passes": 0}


def case_id(c):
    return c[0]


def is_fuzzy(tree):
    return tree is not None and any(n[0] in UNFUZZED for n in tree)


_frames = {}


def oracle_frame(O, R, asset, case):
    """(accumulator (W*H, 4), ARGB (W*H,)) of the case's passes into a cleared framebuffer.  Computed once per case, shared, never written to."""
    name, mesh, tree, pose, w, h, n_passes, ns, depth, _, _ = case
    key = (mesh, repr(tree), pose, w, h, n_passes, ns, depth)
    if key not in _frames:
        if pose is not None:       # the oracle has no camera: its explicit-ray entry behind the ray model (no counter-stream draws in these trees)
            assert tree is not None and not is_fuzzy(tree)
            a, b = CS.oracle_frame(O, asset, [("mesh", mesh, tree)], CS.cam13(R, pose), w, h, ns, depth, n_passes=n_passes, seed=SEED)
        else:
            s = O.Scene()
            sh = s.add_mesh_obj(asset(mesh + ".obj"))
            if tree is not None:
                s.set_material(sh, tree)
            if is_fuzzy(tree):
                s.set_unitvec_mode(O.UNITVEC_F64)
            fb = O.Framebuffer(w, h)
            for p in range(n_passes):
                s.render_range(fb, 0, w * h - 1, depth, False, p, ns, SEED)
            a, b = fb.read()
        a = np.array(a); b = np.array(b)
        a.setflags(write=False); b.setflags(write=False)
        _frames[key] = (a, b)
    return _frames[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)
