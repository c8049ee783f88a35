"""Ray queries on device buffers (RayTracerScene.trace_closest / trace_occluded over torch tensors) on the GPU: bit for bit the reference's golden
records and the CPU oracle's, byte for byte the existing closest kernel on the same buffers ("query_kernel" 0), any-hit == `shape >= 0`."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, asset

pytestmark = pytest.mark.gpu

import raytracerwin_amd as R  # noqa: E402
import scenes as SC  # noqa: E402
from oracle import oracle as _O  # noqa: E402  (material node arrays only)

torch = pytest.importorskip("torch")

MESHES = ["TorusKnot", "BlenderMonkey", "unitychan"]
SCENES = ["default_nofuzz", "quirk", "shapes", "room", "tris"]
NS = (0, 1, 63, 64, 65, 255, 256, 257, None)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.fixture(scope="module")
def ctx():
    c = R.Context(0, stream=torch.cuda.current_stream().cuda_stream)      # the queries run on torch's current stream
    yield c
    c.close()


def build(ctx, tag):
    s = R.RayTracerScene(ctx)
    if tag in MESHES:
        s.AddShape(R.RMeshShape.Create(asset(tag + ".obj")), R.SurfaceMaterial_Diffuse())
    else:
        for sh in SC.SCENES[tag]():
            mat = None if sh[-1] is None else R.material_nodes_from_array(_O.materials(sh[-1]))
            mk = {"sphere": lambda: R.RSphere.Create(sh[1], sh[2]), "plane": lambda: R.RPlane.Create(sh[1], sh[2]), "capsule": lambda: R.RCapsule.Create(sh[1], sh[2], sh[3]),
                  "triangle": lambda: R.RTriangle.Create(sh[1], sh[2], sh[3]), "mesh": lambda: R.RMeshShape.Create(asset(sh[1] + ".obj"))}
            s.AddShape(mk[sh[0]](), mat)
    s.commit()
    return s


@pytest.fixture(scope="module")
def scenes(ctx):
    built = {}

    def get(tag):
        if tag not in built:
            built[tag] = build(ctx, tag)
        return built[tag]
    yield get
    for s in built.values():
        s.close()


def golden(tag):
    return np.load(os.path.join(GOLDEN, ("closest_%s.npz" if tag in MESHES else "sceneclosest_%s.npz") % tag))


def run(ctx, s, rays_t, qk=1, qb=0, prune=1):
    ctx.set_option("query_kernel", qk)
    ctx.set_option("query_blocks", qb)
    s.set_prune(prune)
    hits, shape, tri = s.trace_closest(rays_t)
    occ = s.trace_occluded(rays_t)
    torch.cuda.synchronize()
    ctx.set_option("query_kernel", -1)
    ctx.set_option("query_blocks", 0)
    s.set_prune(1)
    return hits.cpu().numpy(), shape.cpu().numpy(), tri.cpu().numpy(), occ.cpu().numpy()


def check(out, g, n):
    hits, shape, tri, occ = out
    assert hits.shape == (n, 11) and shape.shape == (n,) and tri.shape == (n,) and occ.shape == (n,) and occ.dtype == np.uint8
    assert (shape == g["shape"][:n]).all()
    hit = shape >= 0
    assert (occ == hit.astype(np.uint8)).all()
    assert same(hits[hit], g["hit"][:n][hit])
    if "tri" in g:
        assert (tri[hit] == g["tri"][:n][hit]).all()


@pytest.mark.parametrize("tag", MESHES + SCENES)
def test_device_queries_equal_the_reference_golden(ctx, scenes, tag):
    """every n (batch edges 63 / 64 / 65, block edges 255 / 256 / 257, all), few blocks (several trips of the batch loop) and the default grid,
    prune on and off, both kernels: the reference's records; the two kernels agree on every byte, misses included"""
    g = golden(tag)
    g = {k: g[k] for k in g.files if k != "scene"}
    s = scenes(tag)
    dev = torch.from_numpy(np.ascontiguousarray(g["rays"], np.float32)).cuda()
    for n in NS:
        n = len(g["rays"]) if n is None else n
        rays_t = dev[:n].contiguous()
        for qb in (0, 2):
            for prune in (0, 1):
                new = run(ctx, s, rays_t, 1, qb, prune)
                check(new, g, n)
                old = run(ctx, s, rays_t, 0, qb, prune)
                for a, b in zip(new, old):
                    assert a.tobytes() == b.tobytes()
        for a, b in zip(new, run(ctx, s, rays_t, -1)):         # the default: whichever kernel the measured rule picks for this scene
            assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", MESHES)
def test_device_queries_equal_the_oracle_on_fresh_rays(ctx, scenes, oracle_mod, name):
    """make_rays' seeded rays (camera, interior, axis-parallel, near-epsilon) plus eight odd ones (NaN, inf, zero direction, zero and negative distance)
    against the oracle; unitychan's odd rays (NaN uv at the texture sampler: nothing defined to compare with) only have to be survived"""
    from tests.golden.make_golden import make_rays
    os_ = oracle_mod.Scene()
    sh = os_.add_mesh_obj(asset(name + ".obj"))
    rays = make_rays(os_.shape_bounds(sh), 1500 if name == "unitychan" else 6000, np.random.default_rng(99))
    odd = rays[:8].copy()
    odd[0, 3] = np.nan; odd[1, 5] = np.nan; odd[2, 0] = np.inf; odd[3, 3:6] = 0; odd[4, 6] = 0; odd[5, 6] = -1; odd[6, 4] = 1e-8; odd[7, 3] = np.inf
    s = scenes(name)
    if name == "unitychan":
        run(ctx, s, torch.from_numpy(np.ascontiguousarray(odd, np.float32)).cuda())
    else:
        rays = np.concatenate([rays, odd])
    of, oshape, otri = os_.trace_closest(rays)
    g = {"rays": rays, "hit": of, "shape": oshape, "tri": otri}
    rays_t = torch.from_numpy(np.ascontiguousarray(rays, np.float32)).cuda()
    for prune in (0, 1):
        check(run(ctx, s, rays_t, 1, 0, prune), g, len(rays))


def test_a_batch_larger_than_a_default_grid_sweep(ctx, scenes):
    """2 x (default grid's lanes) + 37 rays: every wave of the default grid loops; the oracle's records on the first 2 700, the old kernel's on all"""
    g = golden("TorusKnot")
    s = scenes("TorusKnot")
    ctx.set_option("query_kernel", 1)
    threads, blocks = s.query_launch_shape(10 ** 9)
    n = 2 * threads * blocks + 37
    assert s.query_launch_shape(n) == (threads, blocks)
    reps = -(-n // len(g["rays"]))
    rays_t = torch.from_numpy(np.ascontiguousarray(g["rays"], np.float32)).cuda().repeat(reps, 1)[:n].contiguous()
    new = run(ctx, s, rays_t, 1)
    check(tuple(a[:2700] for a in new), {k: g[k] for k in g.files}, 2700)
    old = run(ctx, s, rays_t, 0)
    for a, b in zip(new, old):
        assert a.tobytes() == b.tobytes()


def test_outputs_switched_off_are_not_written(ctx, scenes):
    g = golden("quirk")
    s = scenes("quirk")
    n = 1000
    rays_t = torch.from_numpy(np.ascontiguousarray(g["rays"][:n], np.float32)).cuda()
    # one allocation: [shape | neighbour]; only shape is asked for
    pool = torch.full((2 * n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    for qk in (1, 0):
        ctx.set_option("query_kernel", qk)
        pool.fill_(0x5A5A5A5A)
        hits, shape, tri = s.trace_closest(rays_t, hits=False, shape=pool[:n], tri=False)
        torch.cuda.synchronize()
        assert hits is None and tri is None and shape.data_ptr() == pool.data_ptr()
        assert (pool[:n].cpu().numpy() == g["shape"][:n]).all()
        assert (pool[n:] == 0x5A5A5A5A).all().item()
    ctx.set_option("query_kernel", -1)
    fpool = torch.full((n * 11 + n,), 7.25, dtype=torch.float32, device="cuda")
    hits, shape, tri = s.trace_closest(rays_t, hits=fpool[:n * 11], shape=False, tri=False)
    torch.cuda.synchronize()
    assert shape is None and tri is None
    hit = g["shape"][:n] >= 0
    assert same(fpool[:n * 11].cpu().numpy().reshape(n, 11)[hit], g["hit"][:n][hit])
    assert (fpool[n * 11:] == 7.25).all().item()


def test_shadow_rays_built_on_the_device_from_the_first_query(ctx, scenes):
    """two calls back to back on one stream, the second reading the first's hit positions: the host path fed the same rays gives the same bytes"""
    g = golden("default_nofuzz")
    s = scenes("default_nofuzz")
    rays_t = torch.from_numpy(np.ascontiguousarray(g["rays"], np.float32)).cuda()
    hits, shape, _ = s.trace_closest(rays_t)
    light = torch.tensor([3.0, 6.0, 4.0], device="cuda")
    origin = hits[:, 0:3] + hits[:, 3:6] * 1e-3
    to_light = light - origin
    dist = to_light.norm(dim=1, keepdim=True)
    shadow = torch.cat([origin, to_light / dist, dist], dim=1)[shape >= 0].contiguous()
    occ = s.trace_occluded(shadow)
    torch.cuda.synchronize()
    host = s.trace_occluded(shadow.cpu().numpy())
    assert isinstance(host, np.ndarray) and host.dtype == np.uint8
    assert len(host) > 100 and (occ.cpu().numpy() == host).all() and 0 < int(host.sum()) < len(host)


def test_a_query_does_not_disturb_a_render(ctx, scenes):
    s = scenes("TorusKnot")
    W, H = 96, 54

    def frame():
        fb = R.Framebuffer(ctx, W, H)
        s.render_passes(fb, 10, 0, 1, 4, None, 0, 2, 4, 12345)
        out = fb.read_float(), fb.resolve_argb()
        fb.close()
        return out
    a = frame()
    g = golden("TorusKnot")
    run(ctx, s, torch.from_numpy(np.ascontiguousarray(g["rays"], np.float32)).cuda())
    b = frame()
    assert (bits(a[0]) == bits(b[0])).all() and (a[1] == b[1]).all()


def test_work_counters_of_the_query_kernel(ctx, scenes):
    g = golden("unitychan")
    s = scenes("unitychan")
    rays_t = torch.from_numpy(np.ascontiguousarray(g["rays"], np.float32)).cuda()
    n = len(g["rays"])
    ctx.stats_enable(True)
    try:
        ctx.stats_reset()
        s.trace_closest(rays_t)
        torch.cuda.synchronize()
        c = ctx.stats()
        ctx.stats_reset()
        s.trace_occluded(rays_t)
        torch.cuda.synchronize()
        a = ctx.stats()
    finally:
        ctx.stats_enable(False)
    hits = int((g["shape"] >= 0).sum())
    assert c["rays"] == n and a["rays"] == n and c["shaded_hits"] == hits and 0 < c["tex_samples"] <= hits
    assert a["box_tests"] + a["tri_tests"] <= c["box_tests"] + c["tri_tests"] and a["shaded_hits"] == 0
