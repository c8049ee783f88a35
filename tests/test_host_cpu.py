"""Host-side logic of the product library, runnable without a GPU: the C-ABI library loads and
exports every symbol include/rtwin.h declares, refuses to run without a device (no CPU
fallback), and its parser / tree builder / tables agree with the reference goldens and the oracle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, asset

import raytracerwin_amd as R
from raytracerwin_amd import api


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "rtwin.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = set(re.findall(r"\b(rtw_[a-z0-9_]+)\s*\(", hdr))
    assert len(names) >= 30
    L = R.library()
    missing = [n for n in sorted(names) if not hasattr(L, n)]
    assert not missing, missing


def test_no_device_means_error_not_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(R.RtwError) as e:
        R.Context(0)
    assert e.value.code == -2
    s = R.RayTracerScene(None)
    s.AddShape(R.RMeshShape.Create(asset("TorusKnot.obj")), R.SurfaceMaterial_Diffuse())
    with pytest.raises(R.RtwError) as e:
        s.FindIntersectionWithScene(np.zeros((1, 7), np.float32))
    assert e.value.code == -2


def test_product_path_does_not_touch_the_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "raytracerwin_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h", "Makefile")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt and "liboracle" not in txt and \
                    "rt_oracle" not in txt, f


@pytest.mark.parametrize("name", ["TorusKnot", "BlenderMonkey", "unitychan"])
def test_parser_and_flattened_tree_match_reference(name):
    g = np.load(os.path.join(GOLDEN, "mesh_%s.npz" % name))
    s = R.RayTracerScene(None)
    s.AddShape(R.RMeshShape.Create(asset(name + ".obj")))
    info = s.mesh_info()
    assert [info["points"], info["texcoords"], info["normals"], info["tris"]] == g["counts"][:4].tolist()
    assert (bits(info["bounds"]) == bits(g["shape_bounds"])).all()
    b, skip, tri = s.mesh_nodes()
    assert len(b) == 2 * info["tris"] - 1
    assert (bits(b) == bits(g["tree_bounds"])).all()
    assert (tri == g["tree_tri"]).all()
    # skip links: subtree sizes of a full binary tree in preorder
    n = len(skip)
    assert skip[0] == n
    leaf = tri >= 0
    assert (skip[leaf] == np.arange(n)[leaf] + 1).all()
    internal = np.where(~leaf)[0]
    assert (skip[skip[internal + 1]] == skip[internal]).all()       # right child ends where the parent ends
    ntex = int((g["texinfo"][:, 0] > 0).sum())
    assert info["textures"] == ntex


def test_tables_match_oracle(oracle_mod):
    O = oracle_mod
    rng = np.random.default_rng(0)
    for _ in range(2000):
        a = [int(v) for v in rng.integers(0, 2 ** 32, 4, dtype=np.uint64)]
        assert api.rand31(*a) == O.rand31(*a)
    for i in list(range(64)) + [0xFFFFFE, 12345678, 7777777]:
        assert (bits(api.unit_table_entry(i)) == bits(O.unit_table_entry(i))).all()
    assert (bits(api.gamma_thresholds()) == bits(O.gamma_thresholds())).all()
    assert (bits(api.texel_lut()) == bits(O.texel_lut())).all()


def test_gamma_threshold_staircase_equals_powf_formula(oracle_mod):
    """MakePixelColor(LinearToGamma(c)) (libm powf, via the oracle) == number of thresholds <= c,
    which is what the device evaluates instead of calling a device powf."""
    thr = api.gamma_thresholds().astype(np.float32)
    assert (np.diff(thr) > 0).all()
    rng = np.random.default_rng(1)
    c = np.concatenate([rng.random(300000, dtype=np.float32), thr, np.nextafter(thr, np.float32(0)),
                        np.nextafter(thr, np.float32(2)), np.float32([0, 1, 1.5, -0.5, 1e-30, np.inf, 3e38, -0.0])])
    c = np.resize(c, (len(c) // 3) * 3)
    direct = oracle_mod.make_pixel_colors(c.reshape(-1, 3))
    stair = np.searchsorted(thr, c, side="right") - 1
    stair = np.where(c > 0, np.clip(stair, 0, 255), 0).astype(np.uint32).reshape(-1, 3)
    packed = (np.uint32(255) << 24) | (stair[:, 0] << 16) | (stair[:, 1] << 8) | stair[:, 2]
    assert (direct == packed).all()


def test_png_reader_matches_pillow_and_writer_round_trips(tmp_path):
    from PIL import Image
    for rel in ("unitychan/cheek_00.png", "unitychan/skin_01.png"):
        px = api.png_load(asset(rel))
        ref = np.asarray(Image.open(asset(rel)))
        assert px.shape == ref.shape and (px == ref).all()
    rng = np.random.default_rng(3)
    argb = rng.integers(0, 2 ** 32, 37 * 21, dtype=np.uint64).astype(np.uint32)
    out = str(tmp_path / "o.png")
    api._check(R.library().rtw_png_save_argb(out.encode(), argb.ctypes.data_as(C.c_void_p), 37, 21))
    im = np.asarray(Image.open(out))
    assert im.shape == (21, 37, 3)
    assert (im[..., 0].ravel() == (argb >> 16) & 255).all() and (im[..., 2].ravel() == argb & 255).all()
    with pytest.raises(R.RtwError):
        api.png_load(asset("TorusKnot.obj"))


def test_bad_arguments_are_rejected():
    s = R.RayTracerScene(None)
    with pytest.raises(R.RtwError):
        s.AddShape(R.RMeshShape.Create("/nonexistent/mesh.obj"))
    pts = np.zeros((3, 3), np.float32)
    with pytest.raises(R.RtwError):     # index out of range: the reference would read out of bounds
        s.AddShape(R.RMeshShape.FromArrays(pts, pts, pts, [[0, 1, 5]], [[0, 1, 2]], [[0, 1, 2]]))
    idx = s.AddShape(R.RMeshShape.FromArrays(pts, pts, pts, [[0, 1, 2]], [[0, 1, 2]], [[0, 1, 2]]))
    bad = np.zeros(1, dtype=api.MATERIAL_DTYPE)
    bad[0] = (api.MAT_BLEND, 0, 0, 0, 0.5, 0, 0, 0)     # children must follow the parent
    with pytest.raises(R.RtwError):
        api._check(R.library().rtw_scene_set_material(s.h, idx, bad.ctypes.data_as(C.c_void_p), 1))


def test_empty_mesh_and_ragged_inputs():
    s = R.RayTracerScene(None)
    e = np.zeros((0, 3), np.float32)
    s.AddShape(R.RMeshShape.FromArrays(e, e, e, np.zeros((0, 3), np.int32), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.int32)))
    s.commit()
    assert s.mesh_info()["nodes"] == 0


@pytest.mark.parametrize("name", ["TorusKnot", "BlenderMonkey", "unitychan"])
def test_flat_hierarchy_is_the_reference_leaves_in_preorder_under_unions(name):
    """Level 0 of the flat hierarchy = the reference tree's leaf boxes in preorder, bit for bit (the walk gives each
    leaf's OWN box the reference's test); every entry of level 1 / 2 is the exact union of its 16 children."""
    g = np.load(os.path.join(GOLDEN, "mesh_%s.npz" % name))
    s = R.RayTracerScene(None)
    s.AddShape(R.RMeshShape.Create(asset(name + ".obj")))
    leaf = g["tree_tri"] >= 0
    l0, l1, l2 = s.mesh_flat(0), s.mesh_flat(1), s.mesh_flat(2)
    assert (bits(l0) == bits(g["tree_bounds"].reshape(-1, 6)[leaf])).all()
    for child, parent in ((l0, l1), (l1, l2)):
        assert len(parent) == (len(child) + 15) // 16
        for k in range(len(parent)):
            c = child[16 * k:16 * k + 16]
            assert (parent[k, :3] == c[:, :3].min(axis=0)).all() and (parent[k, 3:] == c[:, 3:].max(axis=0)).all()     # values (+0 == -0)


def _camera_dirs(W, H, xs, ys, ox, oy):
    """ThreadWorker_Render's ray direction (Src/RayTracerProgram.cpp:141-165) in float32, before normalisation
    (normalising scales all three components alike and cannot change which boxes the line meets)."""
    f = np.float32
    aspect = f(W) / f(H)
    dx = -(xs - W // 2).astype(f) / f(W * 2) * aspect
    dy = -(ys - H // 2).astype(f) / f(H * 2)
    d = np.stack([dx + ox.astype(f), dy + oy.astype(f), np.full(len(xs), -0.5, f)], 1)
    return d / np.sqrt((d.astype(np.float64) ** 2).sum(1)).astype(f)[:, None]


@pytest.mark.parametrize("name,W,H,bw,bh,step", [("TorusKnot", 192, 108, 16, 4, 3), ("TorusKnot", 96, 54, 32, 2, 1), ("TorusKnot", 128, 72, 64, 1, 2),
                                                 ("BlenderMonkey", 192, 108, 16, 4, 3), ("unitychan", 192, 108, 16, 4, 29),
                                                 ("TorusKnot", 64, 200, 16, 4, 1), ("BlenderMonkey", 64, 600, 16, 4, 3)])
def test_screen_bins_hold_every_triangle_a_camera_ray_can_accept(name, W, H, bw, bh, step):
    """The bins only have to be a superset of what can be ACCEPTED: for camera rays of every (sampled) pixel -- jitter
    corners, centre and random offsets inside the sub-sample range -- every front-facing triangle the ray passes through
    (float64 ray / triangle test) must be in the pixel's bin; every bin lists leaves only, in ascending (= preorder) order.
    (A leaf left out is one the reference would box- or triangle-test and reject: no result changes.)"""
    g = np.load(os.path.join(GOLDEN, "mesh_%s.npz" % name))
    s = R.RayTracerScene(None)
    s.AddShape(R.RMeshShape.Create(asset(name + ".obj")))
    off, ent = s.mesh_bins(W, H, bw, bh)
    bounds, _, tri = s.mesh_nodes()
    assert len(off) == (W // bw) * (H // bh) + 1
    for b in range(len(off) - 1):
        e = ent[off[b]:off[b + 1]]
        assert (np.diff(e.astype(np.int64)) > 0).all() and (tri[e] >= 0).all()
    leaf_nodes = np.nonzero(tri >= 0)[0]
    P = g["points"].reshape(-1, 3).astype(np.float64)
    idx = g["pidx"].reshape(-1, 3)[tri[leaf_nodes]]
    p0, p1, p2 = P[idx[:, 0]], P[idx[:, 1]], P[idx[:, 2]]
    nrm = np.cross(p1 - p0, p2 - p0)
    o = np.array([0, 0, 7.0])
    facing = ((o - p0) * nrm).sum(1) > 1e-7 * np.maximum(1e-30, np.linalg.norm(nrm, axis=1))     # clearly in front of the plane
    nn = np.int64(len(bounds))
    keys = np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(off.astype(np.int64))) * nn + ent.astype(np.int64)     # (bin, leaf) pairs
    rng = np.random.default_rng(7)
    r = np.float32(1.0) / np.float32(W * 4)
    pix = np.arange(0, W * H, step)
    xs, ys = pix % W, pix // W
    bins = ((ys // bh) * (W // bw) + xs // bw).astype(np.int64)
    offsets = [(-0.25, -0.25), (1.25, -0.25), (-0.25, 1.25), (1.25, 1.25), (0.5, 0.5)] + [tuple(rng.uniform(-0.25, 1.25, 2)) for _ in range(3)]
    e1, e2 = p1 - p0, p2 - p0
    missing, seen = 0, 0
    for fx, fy in offsets:
        d = _camera_dirs(W, H, xs, ys, np.full(len(xs), fx * r), np.full(len(xs), fy * r)).astype(np.float64)
        for c0 in range(0, len(xs), 1024):
            dd = d[c0:c0 + 1024]
            # Moeller-Trumbore, rays (n, 1, 3) x triangles (1, m, 3)
            pv = np.cross(dd[:, None, :], e2[None])
            det = (e1[None] * pv).sum(2)
            ok = np.abs(det) > 1e-14
            inv = np.where(ok, 1.0 / np.where(ok, det, 1.0), 0.0)
            tv = (o - p0)[None]
            u = (tv * pv).sum(2) * inv
            qv = np.cross(tv, e1[None])
            v = (dd[:, None, :] * qv).sum(2) * inv
            t = (e2[None] * qv).sum(2) * inv
            hit = ok & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0) & facing[None]
            pi, li = np.nonzero(hit)
            seen += len(pi)
            missing += int((~np.isin(bins[c0 + pi] * nn + leaf_nodes[li], keys)).sum())
    assert seen > 0 and missing == 0


def test_meshes_reaching_behind_the_camera_get_no_bins(tmp_path):
    """A leaf box that is not wholly in front of the camera (z >= 7) cannot be binned: the mesh then has no bins and the
    primary kernel walks its tree instead."""
    p = tmp_path / "near.obj"
    p.write_text("v 0 0 6\nv 1 0 8\nv 0 1 6\nvt 0 0\nvn 0 0 1\nf 1/1/1 2/1/1 3/1/1\n")
    s = R.RayTracerScene(None)
    s.AddShape(R.RMeshShape.Create(str(p)))
    assert s.mesh_bins(192, 108, 16, 4) is None
    assert s.mesh_bins(100, 108, 16, 4) is None        # a frame the bins do not tile


def test_analytic_shapes_keep_insertion_order_and_the_reference_culling_boxes(oracle_mod):
    """RSphere / RCapsule boxes are RAabb::ExpandBySphere from the default box (Src/RAabb.h:46-54, Src/Shapes.h:52,91-92); a plane's
    stays the default inverted box (never consulted: RPlane::HasCullingBounds).  Host-only scene, compared with the oracle's."""
    import scenes as SC
    s = R.RayTracerScene(None)
    o = oracle_mod.Scene()
    shapes = [("sphere", (1.5, 2.5, -2.0), 0.9, None), ("plane", (0.0, 1.0, 0.0), (0.0, -2.0, 0.0), None),
              ("capsule", (-1.5, -1.5, -1.5), (-2.0, -1.5, 0.0), 0.5, None), ("sphere", (0.1, 0.2, 0.3), 1e-3, None)]
    o.add_shapes(shapes, None)
    assert s.AddShape(R.RSphere.Create(shapes[0][1], shapes[0][2])) == 0
    assert s.AddShape(R.RPlane.Create(shapes[1][1], shapes[1][2])) == 1
    assert s.AddShape(R.RCapsule.Create(shapes[2][1], shapes[2][2], shapes[2][3]), R.SurfaceMaterial_Diffuse()) == 2
    assert s.AddShape(R.RSphere.Create(shapes[3][1], shapes[3][2])) == 3
    s.commit()
    for k in range(4):
        info = s.mesh_info(k)
        assert info["tris"] == 0 and info["nodes"] == 0
        assert (info["bounds"].view(np.uint32) == o.shape_bounds(k).view(np.uint32)).all(), k
    assert len(SC.default_scene()) == 7
    with pytest.raises(R.RtwError):
        s.AddShape(R.RSphere.Create((0, 0, 0), 1.0))        # committed


def test_bench_output_dump_is_float32_bounded_and_the_same_rows_every_time(tmp_path):
    """bench.py's dump_outputs: a 1080p frame is written whole (count as a number, R G B bytes of the ARGB word); a 4K frame is cut down to
    a seeded choice of pixels that fits 64 MB, the same rows in both files and in every run; without the whole accumulator only the image."""
    import bench
    rng = np.random.default_rng(3)
    for n, whole in ((1920 * 1080, True), (3840 * 2160, True), (3840 * 2160, False)):
        acc = rng.random((n, 4), dtype=np.float32).view(np.uint32)
        acc[:, 3] = 7
        argb = rng.integers(0, 2 ** 32, n, dtype=np.uint32)
        dirs = [str(tmp_path / ("d%d%d%d" % (n, whole, k))) for k in range(2)]
        for d in dirs:
            bench.dump_outputs(d, acc, argb, whole)
        assert sorted(os.listdir(dirs[0])) == (["accum.npy", "image.npy"] if whole else ["image.npy"])
        assert sum(os.path.getsize(os.path.join(dirs[0], f)) for f in os.listdir(dirs[0])) <= 64 * 10 ** 6
        img = np.load(os.path.join(dirs[0], "image.npy"))
        assert img.dtype == np.float32 and (bits(img) == bits(np.load(os.path.join(dirs[1], "image.npy")))).all()
        rgb = np.stack([(argb >> 16) & 255, (argb >> 8) & 255, argb & 255], 1).astype(np.float32)
        if n == 1920 * 1080:
            assert (img == rgb).all()
        else:
            assert len(img) < n and len(img) * (28 if whole else 12) > 63 * 10 ** 6       # nearly all of the 64 MB is used
        if whole:
            a = np.load(os.path.join(dirs[0], "accum.npy"))
            assert a.dtype == np.float32 and len(a) == len(img) and (a[:, 3] == 7).all()
            assert (bits(a) == bits(np.load(os.path.join(dirs[1], "accum.npy")))).all()
            if n == 1920 * 1080:
                assert (bits(a[:, :3]) == acc[:, :3]).all()
            else:       # the accumulator's rows are the image's rows: find the first one by its colour sums, the image row there must match
                k = int(np.flatnonzero((acc[:, 0] == bits(a[:1, 0])) & (acc[:, 1] == bits(a[:1, 1])))[0])
                assert (rgb[k] == img[0]).all()


def _sanitizer_build():
    import subprocess
    here = os.path.join(ROOT, "tests", "cpu_emul")
    subprocess.check_call(["make", "-C", here, "-j4", "all"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    asan = subprocess.check_output(["/opt/rocm/lib/llvm/bin/clang++", "-print-file-name=libclang_rt.asan-x86_64.so"], text=True).strip()
    assert os.path.exists(asan), asan
    return here, asan


def test_sanitizer_harness_catches_what_it_should():
    """tests/cpu_emul runs GPU threads as fibers and cross-lane operations as rendezvous of a wave (shim/hip/hip_runtime.h, hipemu_rt.cpp).
    Before trusting a clean run of the product under it: a kernel that writes past its buffer, one that reads past the launch's LDS and one
    whose wave splits around a cross-lane operation must each abort; a correct wave-level scan must pass."""
    import subprocess
    here, asan = _sanitizer_build()
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.dirname(asan), ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")
    exe = os.path.join(here, "_build", "selftest")
    r = subprocess.run([exe, "ok"], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "selftest ok" in r.stdout, r.stderr[-2000:]
    for mode, sign in (("oob_global", "heap-buffer-overflow"), ("oob_lds", "heap-buffer-overflow"), ("divergent", "divergent wave operation")):
        r = subprocess.run([exe, mode], capture_output=True, text=True, env=env)
        assert r.returncode != 0 and sign in r.stderr and "unnoticed" not in r.stdout, (mode, r.stderr[-1500:])


def test_product_sources_under_address_and_ub_sanitizers():
    """GPU sanitizers are not available on the pool, so the product's OWN sources -- rtw_device.hip with every kernel of every pipeline and every
    launch wrapper, the device tree / bins build, rtwin_capi.cpp -- are compiled for the host against the HIP stand-in of tests/cpu_emul
    (-fsanitize=address,undefined; "device" buffers and LDS are exactly-sized heap blocks) into librtwin_emul.so, and the Python mirror drives
    it through the same C ABI: frames of single-mesh and multi-shape scenes (pass-batched default pipeline with each of its trace kernels,
    the bins + wave pipeline, the one-thread-per-pixel kernel, ragged frames, texel inheritance, preview), the device build, the query entry
    points.  An out-of-bounds access, an undefined operation or a wave that splits around a cross-lane operation aborts the run; every frame
    must also equal the oracle's bit for bit (the same IEEE operations in the same order, here on x86).  Three processes, ~40 s each."""
    import subprocess
    import sys
    here, asan = _sanitizer_build()
    env = dict(os.environ, RTW_LIB=os.path.join(here, "_build", "librtwin_emul.so"), RTW_TEST_EMULATION="1", LD_PRELOAD=asan,
               ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    groups = [["device_build"], ["textured", "quirk", "setup_scene", "setup_scene_lanes", "room", "tris"], ["mirror", "preview", "ragged", "shapes", "trace_variants", "queries", "split", "workspace"]]
    procs = [subprocess.Popen([sys.executable, os.path.join(here, "emul_cases.py")] + g, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
             for g in groups]
    for g, p in zip(groups, procs):
        out, err = p.communicate(timeout=900)
        assert p.returncode == 0 and ("emul ok: %d cases" % len(g)) in out, (g, out[-1500:], err[-3000:])
        assert "runtime error" not in err and "AddressSanitizer" not in err, err[-3000:]

@pytest.mark.parametrize("world,mode,W,H", [(2, "all", 52, 47), (3, "argb", 50, 47), (3, "all", 48, 20)])
def test_gather_plan_between_ranks_over_the_host_build(tmp_path, oracle_mod, world, mode, W, H):
    """rtw_gather_rows between real processes WITHOUT a GPU (the N > 1 path on the CPU): every rank is a process running the sanitizer harness's
    host build of the product (tests/cpu_emul: the same rtwin_capi.cpp, the same pack / unpack kernel under AddressSanitizer), the transport under
    it is the loopback stand-in for librccl compiled against the same HIP stand-in.  Each rank renders its own 10-row tasks (ragged last task; in
    the 48 x 20 frame rank 2 of 3 owns no task at all), packs them into ONE block, and rank 0 must end up holding, bit for bit, the oracle's frame:
    one message per peer (asserted from rtw_comm_messages), accumulators too in mode "all"."""
    import subprocess
    import sys
    here, asan = _sanitizer_build()
    sup = os.path.join(ROOT, "tests", "support")
    lib = str(tmp_path / "libloopback_emul.so")
    subprocess.run(["/opt/rocm/lib/llvm/bin/clang++", "-O1", "-fPIC", "-shared", "-I" + os.path.join(here, "shim"), os.path.join(sup, "loopback_rccl.cpp"), "-o", lib], check=True)
    env = dict(os.environ, RTW_LIB=os.path.join(here, "_build", "librtwin_emul.so"), RTW_TEST_EMULATION="1", LD_PRELOAD=asan,
               ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1",
               RTW_RCCL_LIBRARY=lib, RTW_LOOPBACK_DIR=str(tmp_path))
    out = str(tmp_path / "rank0.npz")
    procs = [subprocess.Popen([sys.executable, os.path.join(sup, "gather_rank.py"), str(r), str(world), mode, out, str(W), str(H)], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(world)]
    for r, p in enumerate(procs):
        o, e = p.communicate(timeout=600)
        assert p.returncode == 0, (r, o[-1000:], e[-3000:])
        assert "runtime error" not in e and "AddressSanitizer" not in e, e[-3000:]
    ROWS = 10
    n_tasks = (H + ROWS - 1) // ROWS
    owning = [r for r in range(1, world) if r < n_tasks]
    msgs = [int(np.load(out + ".messages%d.npy" % r)[0]) for r in range(world)]
    assert msgs[0] == len(owning) and all(msgs[r] == (1 if r in owning else 0) for r in range(1, world)), msgs      # ONE message per peer
    O = oracle_mod
    os_ = O.Scene()
    sh = os_.add_mesh_obj(asset("TorusKnot.obj"))
    os_.set_material(sh, [(O.MAT_REFLECTIVE, (1, 1, 1), 0, 0, 0)])
    ofb = O.Framebuffer(W, H)
    for p in range(3):
        os_.render_pass_pool(ofb, 3, False, p, 2, 9, threads=0, task_rows=ROWS)
    want_accum, want_argb = ofb.read()
    got = np.load(out)
    assert (got["argb"] == want_argb).all()
    ga = got["accum"]
    if mode == "all":
        assert (bits(ga) == bits(want_accum)).all()
    else:
        mine = (((np.arange(W * H) // W) // ROWS) % world) == 0
        assert (bits(ga[mine]) == bits(want_accum[mine])).all() and (got["accum"][~mine] == 0).all()
