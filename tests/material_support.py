"""Material trees at the edges and limits of the shared evaluation (material_eval / leaf_bounce / leaf_preview), as data: node lists in the
form of tests/scenes.py, (type, rgb, param, child_a, child_b) with children after parents.  TREES maps a name to (nodes, ref): a `ref` tree is
fuzz-free and goes to the reference (tests/golden/matedge_<name>.npz, written by tests/golden/make_golden.py:golden_materials); the others are
compared with the oracle alone, in its f64 unit-vector mode.  Also: the invalid trees rtw_scene_set_material must refuse, a seeded generator of
valid trees wider than tools/soak.py's draws, and the helpers the CPU, emulation and GPU tests share (data and oracle calls only)."""
import numpy as np

from scenes import BL, CO, D, DC, EM, NU, RF, blend, checker, combine, diffuse, emissive, reflective

f32 = np.float32
EPS = float(np.finfo(f32).eps)                                         # FLT_EPSILON: near_zero's switch
BELOW_EPS = float(np.nextafter(f32(EPS), f32(0)))
NAN, INF = float("nan"), float("inf")
MAX_NODES, MAX_BOUNCE = 64, 16                                           # RTW_MAX_MATERIAL_NODES, RTW_MAX_BOUNCE


def null():
    return [(NU, (0, 0, 0), 0, 0, 0)]


_d1, _d2 = diffuse((0.8, 0.7, 0.6)), diffuse((0.2, 0.4, 0.9))
_em, _rf, _dc = emissive((0.3, 0.2, 0.1)), reflective((0.9, 0.8, 0.7)), checker((0.7, 0.9, 0.8), 0.4)


def _chain12():
    """12 nested Blends, mixed factors (0, 1 and out-of-range ones among them), 13 distinct leaves"""
    factors = (0.5, 0.25, 0.75, 0.1, 0.9, 0.5, 0.0, 0.6, 1.0, 0.4, 1.5, 0.5)
    leaf = lambda k: [diffuse, lambda c: checker(c, 0.3 + 0.1 * k), reflective, emissive][k % 4]((0.3 + 0.05 * k, 0.9 - 0.04 * k, 0.5 + 0.03 * (k % 5)))  # noqa: E731
    tree = leaf(12)
    for k in reversed(range(12)):
        tree = blend(leaf(k), tree, factors[k]) if k % 3 else blend(tree, leaf(k), factors[k])
    return tree


def _leaf64(k):
    c = (0.25 + 0.02 * k, 0.95 - 0.02 * k, 0.4 + 0.015 * (k % 7))
    return [(D, c, 0, 0, 0), (DC, c, 0.2 + 0.05 * k, 0, 0), (RF, c, 0, 0, 0), (EM, tuple(0.2 * v for v in c), 0, 0, 0),
            (D, c, 0, 0, 0), (NU, (0, 0, 0), 0, 0, 0), (RF, c, 0, 0, 0), (D, c, 0, 0, 0)][k % 8]


def _nodes64():
    """exactly 64 nodes: a Combine root over a full Blend tree of 63 nodes (31 Blends in heap order, 32 leaves); the root's second child is one
    of that tree's leaves (a node with two parents)"""
    nodes = [(CO, (0, 0, 0), 0, 1, 1 + 31 + 4)]
    for j in range(31):
        nodes.append((BL, (0, 0, 0), (0.5, 0.3, 0.7, 0.45, 0.55)[j % 5], 1 + 2 * j + 1, 1 + 2 * j + 2))
    nodes += [_leaf64(k) for k in range(32)]
    assert len(nodes) == MAX_NODES and nodes[1 + 31 + 4][0] == D
    return nodes


def _build_trees():
    T = {}

    def add(name, nodes, ref=True):
        assert name not in T
        T[name] = (nodes, ref)

    # order and the surviving ray: Combine evaluates B, then A; the ray A wrote is the one that goes on
    add("co_em_d", combine(_em, _d1))
    add("co_d_em", combine(_d1, _em))
    add("co_d_d", combine(_d1, _d2))
    add("co_rf_d", combine(_rf, _d1))
    add("co_nu_d", combine(null(), _d1))
    add("co_em_em", combine(_em, emissive((0.1, 0.3, 0.2))))
    # nesting
    add("co_co", combine(combine(_d1, _em), combine(_rf, _dc)))
    add("bl_co_bl_co", blend(combine(blend(combine(_d1, _em), _rf, 0.5), null()), _dc, 0.3))
    add("chain12", _chain12())
    # sharing and size
    add("co_same_child", [(CO, (0, 0, 0), 0, 1, 1), (D, (0.45, 0.4, 0.35), 0, 0, 0)])
    add("shared_leaf", [(BL, (0, 0, 0), 0.5, 1, 2), (BL, (0, 0, 0), 0.3, 3, 4), (BL, (0, 0, 0), 0.7, 4, 5),
                        (D, (0.8, 0.7, 0.6), 0, 0, 0), (RF, (0.9, 0.8, 0.7), 0, 0, 0), (DC, (0.7, 0.9, 0.8), 0.4, 0, 0)])
    add("nodes64", _nodes64())
    # blend factor: clamped with x < 0 ? 0 : x > 1 ? 1 : x, so NaN stays NaN, and Random() > NaN picks B
    for tag, f in (("m05", -0.5), ("0", 0.0), ("05", 0.5), ("1", 1.0), ("15", 1.5), ("nan", NAN)):
        add("bf_" + tag, blend(_rf, _d2, f))
    # checker size around near_zero's switch (below FLT_EPSILON in magnitude the size counts as 1), negative, huge, infinite
    for tag, s in (("0", 0.0), ("1e_8", 1e-8), ("eps", EPS), ("below_eps", BELOW_EPS), ("m2", -2.0), ("1e_30", 1e-30), ("1e30", 1e30), ("inf", INF),
                   ("1", 1.0)):
        add("ck_" + tag, checker((0.7, 0.9, 0.8), s))
    # albedo channels through all_nonzero
    for tag, g in (("zero", 0.0), ("negzero", -0.0), ("neg", -0.5), ("denorm", 1e-40), ("3", 3.0)):
        add("alb_" + tag, diffuse((0.8, g, 0.6)))
    # infinite and NaN: behind a blend(..., 0.5) with a plain Diffuse, and that behind a Blend that takes it one time in ten, so that most
    # pixels of a frame stay finite
    for tag, g in (("inf", INF), ("nan", NAN)):
        add("alb_" + tag, blend(blend(diffuse((0.8, g, 0.6)), _d1, 0.5), _d2, 0.9))
    add("em_zero", emissive((0.0, 0.0, 0.0)))
    add("em_neg", combine(_d1, emissive((-0.5, 0.2, -0.1))))
    # fuzz: a fuzz <= 0 draws no random numbers; under a Combine the Diffuse sibling and everything after it shift if the count is off
    add("fz_0", reflective((0.9, 0.9, 0.9), 0.0))
    add("co_fz_0", combine(reflective((0.9, 0.9, 0.9), 0.0), _d1))
    for tag, z in (("m1", -1.0), ("1e_30", 1e-30), ("1", 1.0), ("50", 50.0)):
        add("fz_" + tag, reflective((0.9, 0.9, 0.9), z), ref=z <= 0)
        add("co_fz_" + tag, combine(reflective((0.9, 0.9, 0.9), z), _d1), ref=z <= 0)
    return T


TREES = _build_trees()
REF_TREES = sorted(n for n, (_, ref) in TREES.items() if ref)
FUZZY_TREES = sorted(n for n, (_, ref) in TREES.items() if not ref)
ALL_TREES = sorted(TREES)
assert all(nodes[i][2] <= 0 or nodes[i][0] != RF for n in REF_TREES for nodes in [TREES[n][0]] for i in range(len(nodes)))

MESH = "TorusKnot"
SEED = 20261021
FRAME = (48, 27, 2, 5)                                                   # width, height, sub-samples, depth of every matedge frame
DEPTH16 = dict(mesh=MESH, material=reflective((0.9, 0.8, 0.7)), W=48, H=27, ns=1, depth=16, seed=99)       # make_golden's `mirror`


# combine(Emissive, Diffuse): the surviving ray is the incoming one, so a path that hits the mesh hits it at every level down to the last; an
# albedo above 1 keeps the last level's emission visible in the sum through 15 attenuations
DEPTH16_TREE = combine(_em, diffuse((2.5, 2.2, 2.0)))
MATEDGE_SCENE_TREES = ("co_em_d", "co_co", "co_d_d")                    # the trees scene "matedge" of tests/scenes.py carries, shape by shape


# ---- what rtw_scene_set_material must refuse: name -> (nodes, error); nodes as (type, rgb, param, child_a, child_b) ----
ERR_INVALID, ERR_LIMIT = -1, -6


def _co(a, b):
    return (CO, (0, 0, 0), 0, a, b)


def _bl(a, b, f=0.5):
    return (BL, (0, 0, 0), f, a, b)


_L = (D, (0.5, 0.5, 0.5), 0, 0, 0)
INVALID = {
    "zero_nodes": ([], ERR_LIMIT),
    "nodes65": ([_bl(1, 2)] + [_L] * 64, ERR_LIMIT),
    "type_minus1": ([(-1, (1, 1, 1), 0, 0, 0)], ERR_INVALID),
    "type_7": ([_bl(1, 2), _L, (7, (1, 1, 1), 0, 0, 0)], ERR_INVALID),
    "self_loop": ([_bl(0, 1), _L], ERR_INVALID),                         # a Blend that points at itself: a kernel would never leave it
    "self_loop_b": ([_co(1, 0), _L], ERR_INVALID),
    "child_before_parent": ([_bl(1, 2), _bl(0, 2), _L], ERR_INVALID),
    "child_is_n_nodes": ([_bl(1, 2), _L], ERR_INVALID),
    "child_negative": ([_co(-1, 1), _L], ERR_INVALID),
    "combine3_direct": ([_co(1, 4), _co(2, 4), _co(3, 4), _L, _L], ERR_LIMIT),
    "combine3_blends_between": ([_co(1, 6), _bl(2, 6), _co(3, 6), _bl(6, 4), _co(5, 6), _L, _L], ERR_LIMIT),
    # node 3 is a Combine reached at nesting 1 from the root and at nesting 2 through node 1: its own level is then 3
    "combine3_two_parents": ([_co(1, 3), _co(2, 3), _L, _co(4, 5), _L, _L], ERR_LIMIT),
}
# accepted: leaves whose child fields hold garbage (only Blend and Combine read them)
GARBAGE_LEAVES = [_bl(1, 2, 0.5), (D, (0.8, 0.7, 0.6), 0, -7, 1 << 30), (RF, (0.9, 0.8, 0.7), 0, 99, -(1 << 31))]
GARBAGE_CLEAN = [_bl(1, 2, 0.5), (D, (0.8, 0.7, 0.6), 0, 0, 0), (RF, (0.9, 0.8, 0.7), 0, 0, 0)]
PREVIOUS = diffuse((0.6, 0.7, 0.8))                                      # the material a refused call must leave in force


def combine_nesting(nodes):
    """the deepest Combine nesting of a node list (the rule of rtw_scene_set_material, restated), or None if a child does not follow its parent"""
    level = [0] * len(nodes)
    deepest = 0
    for i, (t, _, _, a, b) in enumerate(nodes):
        if t in (BL, CO):
            if not (i < a < len(nodes) and i < b < len(nodes)):
                return None
            d = level[i] + (t == CO)
            deepest = max(deepest, d)
            level[a], level[b] = max(level[a], d), max(level[b], d)
    return deepest


# ---- a seeded family wider than the soak's: composite depth up to the limits, parameters from the edge values mixed with ordinary ones ----
_EDGE_FACTORS = (-0.5, 0.0, 1.0, 1.5, NAN, 0.5, 0.25, 0.9)
_EDGE_SIZES = (0.0, 1e-8, EPS, BELOW_EPS, -2.0, 1e-30, 1e30, INF, 0.3, 1.0, 5.0)
_EDGE_CHANNELS = (0.0, -0.0, -0.5, 1e-40, 3.0)


def random_tree(rng):
    """A valid fuzz-free tree: at most 64 nodes, Combine nesting at most 2 (often exactly 2, on both sides), Blend chains up to 8 deep."""
    nodes = []

    def channel():
        return float(rng.choice(_EDGE_CHANNELS)) if rng.random() < 0.12 else float(f32(rng.uniform(0.05, 1.0)))

    def leaf():
        t = int(rng.choice([D, D, DC, RF, EM, NU]))
        c = (channel(), channel(), channel())
        if t == EM:
            c = tuple(0.3 * v for v in c)
        p = (float(rng.choice(_EDGE_SIZES)) if rng.random() < 0.5 else float(f32(rng.uniform(0.1, 3.0)))) if t == DC else 0.0
        return (t, c, p, 0, 0)

    def grow(combines_left, blends_left, budget):
        """appends a subtree, returns its index; budget: nodes this subtree may still add (>= 1)"""
        me = len(nodes)
        kinds = []
        if budget >= 3:
            if combines_left > 0:
                kinds += [CO, CO]
            if blends_left > 0:
                kinds += [BL, BL]
        if not kinds or rng.random() < 0.15:
            nodes.append(leaf())
            return me
        t = int(rng.choice(kinds))
        nodes.append(None)
        left = (budget - 1) // 2
        args = (combines_left - (t == CO), blends_left - (t == BL))
        a = grow(*args, left)
        b = grow(*args, budget - 1 - left)
        if rng.random() < 0.1:                                           # a shared child
            b = a
        f = (float(rng.choice(_EDGE_FACTORS)) if rng.random() < 0.4 else float(f32(rng.uniform(0.05, 0.95)))) if t == BL else 0.0
        nodes[me] = (t, (0, 0, 0), f, a, b)
        return me

    grow(2, int(rng.integers(0, 9)), int(rng.choice([3, 7, 15, 31, MAX_NODES])))
    return nodes


def random_family(n=40, seed=20261021):
    rng = np.random.default_rng(seed)
    return [random_tree(rng) for _ in range(n)]


# ---- shared helpers (oracle calls and comparisons only) ----
def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    """bit-identical, except that any NaN equals any NaN (the suite's rule: payload and sign of a NaN are not specified)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def oracle_scene(O, asset, material, mesh=MESH, fuzzy=False):
    s = O.Scene()
    sh = s.add_mesh_obj(asset(mesh + ".obj"))
    s.set_material(sh, material)
    if fuzzy:
        s.set_unitvec_mode(O.UNITVEC_F64)
    return s


def oracle_frame(O, scene, W, H, ns, depth, preview=False, n_passes=1, seed=SEED, history=None):
    fb = O.Framebuffer(W, H)
    for p in range(n_passes):
        scene.render_range(fb, 0, W * H - 1, depth, preview, p, ns, seed, history=history)
    return fb.read()


_frames = {}


def oracle_tree_frame(O, asset, name, W, H, ns, depth, preview=False, n_passes=1):
    """the oracle's frame of TREES[name] on the mesh (computed once per argument set, shared, never written to)"""
    key = (name, W, H, ns, depth, preview, n_passes)
    if key not in _frames:
        nodes, ref = TREES[name]
        a, b = oracle_frame(O, oracle_scene(O, asset, nodes, fuzzy=not ref), W, H, ns, depth, preview, n_passes)
        a.setflags(write=False); b.setflags(write=False)
        _frames[key] = (a, b)
    return _frames[key]
