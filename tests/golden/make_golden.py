#!/usr/bin/env python3
"""Generate tests/golden/*.npz from the REAL reference.

Runs oracle/_ref/ref_harness, i.e. the reference's own translation units compiled in
place from /root/reference (oracle/Makefile), with rand() interposed so that every
stochastic decision is replayed from the counter-based generator of the oracle.  The
fixtures hold inputs + the reference's outputs only (no reference text).  Run it in
the build container only; the GPU box never regenerates fixtures.

    python tests/golden/make_golden.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import oracle as O  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scenes as SC  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
ASSETS = os.path.join(ROOT, "assets")
H = O.REF_HARNESS
D, DC, RF, EM, BL, CO, NU = range(7)

MATERIALS = {
    "diffuse": [(D, (1, 1, 1), 0, 0, 0)],
    "mirror": [(RF, (0.9, 0.8, 0.7), 0, 0, 0)],
    "blendfuzz": [(BL, (0, 0, 0), 0.5, 1, 2), (RF, (1, 1, 1), 0.2, 0, 0), (D, (1, 1, 1), 0, 0, 0)],
    "checker": [(DC, (0.8, 0.9, 1.0), 0.3, 0, 0)],
    "combine": [(CO, (0, 0, 0), 0, 1, 4), (BL, (0, 0, 0), 0.5, 2, 3), (RF, (0.95, 0.75, 0.1), 0, 0, 0),
                (D, (0.95, 0.75, 0.1), 0, 0, 0), (EM, (0.475, 0.375, 0.05), 0, 0, 0)],
    "null": [(NU, (0, 0, 0), 0, 0, 0)],
    "partial": [(D, (0.5, 0.0, 0.2), 0, 0, 0)],
    "combine_d16": [(CO, (0, 0, 0), 0, 1, 2), (EM, (0.3, 0.2, 0.1), 0, 0, 0), (D, (2.5, 2.2, 2.0), 0, 0, 0)],     # tests/material_support.py DEPTH16_TREE
}


def obj_path(name):
    return os.path.join(ASSETS, name + ".obj")


def run(args):
    subprocess.check_call([H] + [str(a) for a in args], stdout=subprocess.DEVNULL)


def make_rays(bounds, n, rng):
    lo, hi = bounds[:3].astype(np.float64), bounds[3:].astype(np.float64)
    ext = hi - lo
    rays = []
    tgt = lo + rng.random((n, 3)) * ext                      # camera rays through the mesh box
    o = np.tile(np.array([0, 0, 7.0]), (n, 1))
    d = tgt - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays.append(np.c_[o, d, np.full(n, 1000.0)])
    o = lo + rng.random((n, 3)) * ext                        # interior origins, random directions (secondary-like)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays.append(np.c_[o, d, rng.uniform(0.5, 1000, n)])
    k = max(n // 4, 1)
    o = lo + rng.random((k, 3)) * ext                        # axis-parallel (-z, +x): slab axes skipped
    o[:, 2] = hi[2] + 1
    rays.append(np.c_[o, np.tile([0, 0, -1.0], (k, 1)), np.full(k, 50.0)])
    o = lo + rng.random((k, 3)) * ext
    o[:, 0] = lo[0] - 1
    rays.append(np.c_[o, np.tile([1.0, 0, 0], (k, 1)), np.full(k, 50.0)])
    o = lo + rng.random((k, 3)) * ext                        # near-zero components around FLT_EPSILON
    o[:, 1] = hi[1] + 0.5
    d = np.c_[rng.uniform(-1e-6, 1e-6, k), -np.ones(k), rng.uniform(-2e-7, 2e-7, k)]
    rays.append(np.c_[o, d, np.full(k, 10.0)])
    o = lo + rng.random((k, 3)) * ext                        # short segments that end inside the mesh
    d = rng.normal(size=(k, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays.append(np.c_[o, d, rng.uniform(0.01, 0.3, k)])
    return np.concatenate(rays).astype(np.float32)


# ---- rays aimed at the edges of the analytic shapes (scene "edges" of tests/scenes.py) ----
EDGE_FAMILIES = ("generic", "centre", "from_centre", "surface_in", "surface_out", "tangent", "segment_end",
                 "plane_parallel", "plane_inside", "plane_near_parallel", "plane_origin_on", "plane_behind",
                 "capsule_axis", "capsule_parallel", "capsule_seam", "capsule_perp_end",
                 "tri_vertex", "tri_edge", "tri_behind", "tri_inplane", "odd")
EDGE_ULP_FAMILIES = ("tangent", "segment_end", "capsule_parallel", "capsule_seam", "tri_vertex", "tri_edge")   # hit or miss decided within a few ulps
EDGE_ULPS = (0, 1, 2, 8, 1000)
EDGE_DISTANCE_ULPS = (0, 1, -1, 4, -4)
ULP = 2.0 ** -23


def _step32(x, k):
    """the float32 value k representable steps above (k > 0) or below (k < 0) float32(x)"""
    x = np.float32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf), dtype=np.float32)
    return x


def make_edge_rays(scene, rng):
    """Rays drawn per shape of `scene` at the places where a shape test decides within a few ulps: (rays (n, 7) float32,
    family (n,) int32 indices into EDGE_FAMILIES, target (n,) int32 shape index the ray was aimed at)."""
    out = []                                                        # (origin, direction, distance, family, target)

    def emit(fam, tgt, o, d, dist=1000.0):
        out.append((np.asarray(o, np.float64), np.asarray(d, np.float64), float(dist), EDGE_FAMILIES.index(fam), tgt))

    def unit(v):
        return v / np.linalg.norm(v)

    def rand_unit(towards=None, least=0.3):
        while True:
            u = unit(rng.normal(size=3))
            if towards is None or u @ towards >= least:
                return u

    def perp(u):
        while True:
            w = np.cross(u, rng.normal(size=3))
            if np.linalg.norm(w) > 1e-3:
                return unit(w)

    def basis(n):
        """two unit vectors that span the plane of normal n; exact axes for an axis-aligned n"""
        k = int(np.argmax(np.abs(n)))
        if abs(abs(n[k]) - 1.0) < 1e-12:
            return np.eye(3)[(k + 1) % 3], np.eye(3)[(k + 2) % 3]
        t1 = unit(np.cross(n, np.eye(3)[(k + 1) % 3]))
        return t1, np.cross(n, t1)

    def sphere_like(tgt, c, radius, hemi=None, generic=10):
        """a sphere, or a capsule's end cap (hemi: the axis direction that points out of the capsule there)"""
        c, r = np.asarray(c, np.float64), abs(float(radius))
        size = max(r, 0.25)
        for _ in range(4):
            u = rand_unit(hemi)
            emit("centre", tgt, c + u * (r + size * rng.uniform(1, 4)), -u)
        for _ in range(2):
            emit("from_centre", tgt, c, rand_unit(hemi))
        for _ in range(3):
            u = rand_unit(hemi)
            emit("surface_in", tgt, c + u * r, -u)
            u = rand_unit(hemi)
            emit("surface_out", tgt, c + u * r, u)
        for j in EDGE_ULPS:                                         # closest approach to the centre: radius * (1 +- j * 2^-23)
            for s in (1.0, -1.0):
                for _ in range(6):
                    u = rand_unit(hemi)
                    w = perp(u)
                    p = c + u * (r * (1.0 + s * j * ULP))
                    emit("tangent", tgt, p - w * (size * rng.uniform(1, 3)), w)
        for k in EDGE_DISTANCE_ULPS:                                # a segment that ends at the analytic hit distance, moved by k ulps
            for _ in range(6):
                u = rand_unit(hemi)
                o = (c + u * (r + size * rng.uniform(1, 4))).astype(np.float32).astype(np.float64)
                emit("segment_end", tgt, o, -u, _step32(np.linalg.norm(o - c) - r, k))
        for _ in range(generic):
            o = c + rand_unit(hemi, -1.0) * (r + size * rng.uniform(1, 4))
            emit("generic", tgt, o, unit(c + rand_unit() * (size * rng.uniform(0, 2.5)) - o), rng.uniform(0.5, 8) * size)

    for tgt, sh in enumerate(scene):
        if sh[0] == "sphere":
            sphere_like(tgt, sh[1], sh[2])
        elif sh[0] == "plane":
            n, p = np.asarray(sh[1], np.float64), np.asarray(sh[2], np.float64)
            nn = unit(n) if np.linalg.norm(n) > 0 else np.array([0.0, 1.0, 0.0])        # a zero normal: aimed at as if it were a y-plane
            t1, t2 = basis(nn)
            on = lambda: p + t1 * rng.uniform(-4, 4) + t2 * rng.uniform(-4, 4)           # noqa: E731
            inside = lambda: (lambda a: t1 * np.cos(a) + t2 * np.sin(a))(rng.uniform(0, 2 * np.pi))   # noqa: E731
            for _ in range(4):
                emit("plane_parallel", tgt, on() + nn * rng.uniform(0.5, 2), inside())
                emit("plane_inside", tgt, on(), inside())
            for j in (1, 2, 4, 5, 8, 1000):                         # |normal . direction| around the test's 1e-6
                for side in (1.0, -1.0):
                    for heading in (1.0, -1.0):
                        for _ in range(2):
                            emit("plane_near_parallel", tgt, on() + nn * (side * rng.uniform(0.5, 2)), unit(inside() - nn * (heading * j * ULP)), 1e30)
            for _ in range(6):
                emit("plane_origin_on", tgt, on(), rand_unit())
            for _ in range(4):
                emit("plane_behind", tgt, on() - nn * rng.uniform(0.5, 2), rand_unit(nn))
                emit("plane_behind", tgt, on() - nn * rng.uniform(0.5, 2), -rand_unit(nn))
            for k in EDGE_DISTANCE_ULPS:
                for _ in range(4):
                    o = (on() + nn * rng.uniform(0.5, 2)).astype(np.float32).astype(np.float64)
                    d = -rand_unit(nn)
                    emit("segment_end", tgt, o, d, _step32(((p - o) @ nn) / (d @ nn), k))
            for _ in range(10):
                emit("generic", tgt, on() + nn * rng.uniform(-2, 2), rand_unit(), rng.uniform(0.5, 8))
        elif sh[0] == "capsule":
            a, b, r = np.asarray(sh[1], np.float64), np.asarray(sh[2], np.float64), float(sh[3])
            length = np.linalg.norm(b - a)
            e = unit(b - a) if length > 0 else np.array([0.0, 0.0, 1.0])
            size = max(r, 0.25)
            sphere_like(tgt, a, r, -e, generic=0)
            sphere_like(tgt, b, r, e, generic=0)
            for end, out_dir in ((a, -e), (b, e)):
                emit("capsule_axis", tgt, end + out_dir * (r + rng.uniform(1, 3)), -out_dir)                                # along the axis, through both caps
                emit("capsule_axis", tgt, end + out_dir * (r + rng.uniform(1, 3)) + perp(e) * (r * 0.5), -out_dir)
                for j in EDGE_ULPS:
                    for s in (1.0, -1.0):
                        for _ in range(2):
                            w = perp(e)
                            emit("capsule_parallel", tgt, end + out_dir * (r + rng.uniform(0.5, 2)) + w * (r * (1.0 + s * j * ULP)), -out_dir)
                            # tangent to the surface at a point of the seam between side and cap, heading anywhere in the tangent plane
                            w, ang = perp(e), rng.uniform(0, 2 * np.pi)
                            d = unit(e * np.cos(ang) + np.cross(e, w) * np.sin(ang))
                            emit("capsule_seam", tgt, end + w * (r * (1.0 + s * j * ULP)) - d * (size * rng.uniform(1, 3)), d)
                for j in (0, 1, -1, 8, -8):                         # perpendicular to the axis at its end, a few ulps to either side of the seam
                    w = perp(e)
                    emit("capsule_perp_end", tgt, end + e * (j * ULP * max(length, 1.0)) + w * (r + size * rng.uniform(1, 3)), -w)
            for _ in range(10):
                o = a + (b - a) * rng.uniform(-0.2, 1.2) + rand_unit() * (r + size * rng.uniform(1, 4))
                emit("generic", tgt, o, unit(a + (b - a) * rng.uniform(-0.2, 1.2) + rand_unit() * (size * rng.uniform(0, 2.5)) - o), rng.uniform(0.5, 8) * size)
        elif sh[0] == "triangle":
            v = [np.asarray(q, np.float64) for q in sh[1:4]]
            n = unit(np.cross(v[1] - v[0], v[2] - v[0]))            # the side the reference sees it from
            g = (v[0] + v[1] + v[2]) / 3.0
            step = 4.0 * ULP                                         # coordinates of magnitude 2 - 4: one ulp of a position
            front = lambda aim: aim + n * rng.uniform(1, 3) + perp(n) * rng.uniform(0, 0.5)     # noqa: E731
            for i in range(3):
                mid = (v[i] + v[(i + 1) % 3]) / 2.0
                outward = unit(np.cross(v[(i + 1) % 3] - v[i], n))
                for j in EDGE_ULPS:
                    for s in (1.0, -1.0):
                        for _ in range(2):
                            aim = v[i] + unit(v[i] - g) * (s * j * step)
                            o = front(aim)
                            emit("tri_vertex", tgt, o, unit(aim - o))
                            aim = mid + outward * (s * j * step)
                            o = front(aim)
                            emit("tri_edge", tgt, o, unit(aim - o))
            for _ in range(3):
                o = g - n * rng.uniform(1, 3) + perp(n) * rng.uniform(0, 0.3)
                emit("tri_behind", tgt, o, unit(g - o))
                w = perp(n)
                emit("tri_inplane", tgt, g + w * 3.0, -w)
            emit("tri_inplane", tgt, g, -n)                          # origin in the triangle, looking down and up
            emit("tri_inplane", tgt, g, n)
            for k in EDGE_DISTANCE_ULPS:
                for _ in range(4):
                    o = front(g).astype(np.float32).astype(np.float64)
                    d = unit(g - o)
                    emit("segment_end", tgt, o, d, _step32(((v[0] - o) @ n) / (d @ n), k))
            for _ in range(10):
                o = g + rand_unit() * rng.uniform(1, 4)
                emit("generic", tgt, o, unit(g + rand_unit() * rng.uniform(0, 2) - o), rng.uniform(0.5, 8))
        else:
            bounds = np.load(os.path.join(OUT, "mesh_%s.npz" % sh[1]))["shape_bounds"]
            for ray in make_rays(bounds, 40, rng):
                emit("generic", tgt, ray[:3], ray[3:6], ray[6])
    # the odd rays, sent at one shape of each kind (the last of its kind in the list): a ray that hits it, spoiled in one way
    last = {sh[0]: k for k, sh in enumerate(scene)}
    for kind, tgt in sorted(last.items()):
        sh = scene[tgt]
        if kind == "plane":
            tgt = max(k for k, s in enumerate(scene) if s[0] == "plane" and np.linalg.norm(s[1]) > 0)
            sh = scene[tgt]
            aim, o = np.asarray(sh[2], np.float64), np.asarray(sh[2], np.float64) + unit(np.asarray(sh[1], np.float64)) * 2 + np.array([0.3, 0.0, 0.2])
        elif kind == "mesh":
            aim, o = np.array([0.0, 0.0, 0.0]), np.array([0.5, 0.3, 6.0])
        elif kind == "triangle":
            v = [np.asarray(q, np.float64) for q in sh[1:4]]
            aim = (v[0] + v[1] + v[2]) / 3.0
            o = aim + unit(np.cross(v[1] - v[0], v[2] - v[0])) * 2
        else:
            aim = np.asarray(sh[1], np.float64) if kind == "sphere" else (np.asarray(sh[1], np.float64) + np.asarray(sh[2], np.float64)) / 2
            o = aim + np.array([0.4, 0.5, 3.0])
        d = unit(aim - o)
        nan, inf = np.nan, np.inf
        emit("odd", tgt, o, d)                                       # (the unspoiled ray)
        emit("odd", tgt, o * [1, nan, 1], d)
        emit("odd", tgt, o, d * [1, 1, nan])
        emit("odd", tgt, o + [inf, 0, 0], d)
        emit("odd", tgt, o, d + [0, inf, 0])
        emit("odd", tgt, o, d * 0)
        emit("odd", tgt, o, d, 0.0)
        emit("odd", tgt, o, d, -1.0)
        emit("odd", tgt, o, d, 1e-40)
        emit("odd", tgt, o, d * 1e-3)
        emit("odd", tgt, o, d * 1e3)
    rays = np.array([np.r_[o, d, dist] for o, d, dist, _, _ in out]).astype(np.float32)
    return rays, np.array([f for *_, f, _ in out], np.int32), np.array([t for *_, t in out], np.int32)


def golden_mesh(name, tmp):
    pre = os.path.join(tmp, name)
    run(["dump_mesh", obj_path(name), pre])
    f32 = lambda s: np.fromfile(pre + s, np.float32)  # noqa: E731
    i32 = lambda s: np.fromfile(pre + s, np.int32)  # noqa: E731
    np.savez_compressed(os.path.join(OUT, "mesh_%s.npz" % name),
                        counts=i32(".counts.i32"), points=f32(".points.f32").reshape(-1, 3),
                        texcoords=f32(".texcoords.f32").reshape(-1, 3), normals=f32(".normals.f32").reshape(-1, 3),
                        pidx=i32(".pidx.i32").reshape(-1, 3), tidx=i32(".tidx.i32").reshape(-1, 3),
                        nidx=i32(".nidx.i32").reshape(-1, 3), matid=i32(".matid.i32"),
                        tree_bounds=f32(".tree_bounds.f32").reshape(-1, 6), tree_tri=i32(".tree_tri.i32"),
                        shape_bounds=f32(".shape_bounds.f32"), texinfo=i32(".texinfo.i32").reshape(-1, 2))
    return f32(".shape_bounds.f32")


def golden_closest(name, bounds, n, tmp, rng):
    rays = make_rays(bounds, n, rng)
    rp, hp = os.path.join(tmp, "rays.bin"), os.path.join(tmp, "hits.bin")
    rays.tofile(rp)
    run(["closest", obj_path(name), rp, len(rays), hp])
    r = np.fromfile(hp, np.float32).reshape(-1, 13)
    np.savez_compressed(os.path.join(OUT, "closest_%s.npz" % name), rays=rays, hit=r[:, :11].copy(),
                        shape=r[:, 11].copy().view(np.int32), tri=r[:, 12].copy().view(np.int32))


def golden_texsample(name, mat, n, tmp, rng):
    uv = rng.uniform(-2.5, 2.5, (n, 2)).astype(np.float32)
    edge = np.array([[0, 0], [1, 1], [0.5, 0.5], [-1e-9, 0.25], [0.25, -1e-9], [1.0, 0.0], [0.999999, 0.999999],
                     [2.0, -3.0], [1 / 511.0, 2 / 511.0], [255 / 255.0, 17 / 255.0]], np.float32)
    uv = np.concatenate([edge, uv])
    up, op = os.path.join(tmp, "uv.bin"), os.path.join(tmp, "tex.bin")
    uv.tofile(up)
    run(["texsample", obj_path(name), mat, up, len(uv), op])
    np.savez_compressed(os.path.join(OUT, "texsample_%s_m%d.npz" % (name, mat)), uv=uv, material=np.int32(mat),
                        rgba=np.fromfile(op, np.float32).reshape(-1, 4))


def golden_frame(tag, name, mat, W, Hh, ns, depth, preview, seed, pass0, npass, tmp):
    arr = O.materials(MATERIALS[mat])
    mp, fp = os.path.join(tmp, "mat.bin"), os.path.join(tmp, "frame")
    arr.tofile(mp)
    run(["frame", obj_path(name), mp, W, Hh, ns, depth, preview, seed, pass0, npass, 0, W * Hh - 1, fp])
    np.savez_compressed(os.path.join(OUT, "frame_%s.npz" % tag), mesh=name, material=arr,
                        params=np.array([W, Hh, ns, depth, preview, seed, pass0, npass], np.int64),
                        accum=np.fromfile(fp + ".accum.f32", np.float32).reshape(-1, 4),
                        argb=np.fromfile(fp + ".argb.u32", np.uint32))


def golden_worker(tag, name, mat, depth, preview, seed, pass0, npass, tmp):
    """The reference's OWN ThreadWorker_Render (Src/RayTracerProgram.cpp:131-188; 800 x 800, 4 sub-samples) writing its own accuBuffer[] /
    bitcolor[] (harness command `worker`).  Kept: the whole ARGB image, the SHA-256 of the accumulator's bytes (count as int32) and the
    accumulator of a 64-row band."""
    import hashlib
    W = Hh = 800
    arr = O.materials(MATERIALS[mat])
    mp, fp = os.path.join(tmp, "mat.bin"), os.path.join(tmp, "worker")
    arr.tofile(mp)
    run(["worker", obj_path(name), mp, depth, preview, seed, pass0, npass, 0, W * Hh - 1, fp])
    accum = np.fromfile(fp + ".accum.f32", np.float32).reshape(-1, 4)
    ints = accum.copy()
    ints[:, 3] = accum[:, 3].astype(np.int32).view(np.float32)          # the count as the int the reference holds
    band = slice(368 * W, 432 * W)
    np.savez_compressed(os.path.join(OUT, "worker_%s.npz" % tag), mesh=name, material=arr,
                        params=np.array([W, Hh, 4, depth, preview, seed, pass0, npass], np.int64),
                        argb=np.fromfile(fp + ".argb.u32", np.uint32), accum_sha256=hashlib.sha256(ints.tobytes()).hexdigest(),
                        band=np.array([368, 432], np.int64), accum_band=accum[band])


def golden_misc(tmp):
    """Small facts straight from the reference's own functions: FormatTimeString's renderings (Src/RayTracerProgram.cpp:242-268) and a PNG
    written by RTexture::SaveBufferToPNG (Src/Texture.cpp:201-283) with its decoded pixels."""
    import json
    from PIL import Image
    ms = [0, 1, 999, 1000, 1001, 59999, 60000, 61000, 125000, 3599999, 3600000, 3661000, 3725000, 86400000 + 62000]
    out = subprocess.check_output([H, "timestring"] + [str(v) for v in ms]).decode().strip().splitlines()
    table = {int(ln.split(" ", 1)[0]): ln.split(" ", 1)[1] for ln in out}
    json.dump(table, open(os.path.join(OUT, "timestrings.json"), "w"), indent=0, sort_keys=True)
    g = np.load(os.path.join(OUT, "frame_unitychan_diffuse_d4.npz"))
    W, Hh = int(g["params"][0]), int(g["params"][1])
    argb = g["argb"].astype(np.uint32)
    ap, pp = os.path.join(tmp, "img.argb"), os.path.join(OUT, "png_written_by_reference.png")
    argb.tofile(ap)
    run(["savepng", ap, W, Hh, pp])
    np.savez_compressed(os.path.join(OUT, "png_reference_decode.npz"), argb=argb, size=np.array([W, Hh]), rgb=np.asarray(Image.open(pp).convert("RGB")))


def main_worker(tmp):
    golden_worker("torus_mirror_d4", "TorusKnot", "mirror", 4, 0, 31, 0, 2, tmp)
    golden_worker("unitychan_preview", "unitychan", "diffuse", 4, 1, 31, 0, 1, tmp)
    golden_worker("unitychan_mirror_d3", "unitychan", "mirror", 3, 0, 77, 1, 1, tmp)


def golden_raytrace(tag, name, mat, n, depth, seed, W, Hh, tmp, rng, bounds):
    rays = make_rays(bounds, n, rng)
    keys = np.c_[rng.integers(0, W * Hh, len(rays)), rng.integers(0, 8, len(rays))].astype(np.uint32)
    arr = O.materials(MATERIALS[mat])
    mp, rp, kp, op = [os.path.join(tmp, f) for f in ("mat.bin", "rays.bin", "keys.bin", "rt.bin")]
    arr.tofile(mp)
    rays.tofile(rp)
    keys.tofile(kp)
    run(["raytrace", obj_path(name), mp, rp, kp, len(rays), depth, 0, seed, W, Hh, op])
    np.savez_compressed(os.path.join(OUT, "raytrace_%s.npz" % tag), mesh=name, material=arr, rays=rays, keys=keys,
                        params=np.array([depth, seed, W, Hh], np.int64),
                        rgb=np.fromfile(op, np.float32).reshape(-1, 3))


def write_scene_file(scene, tmp, tag):
    """the harness's .scene text: shapes in insertion order, numbers as exact decimal renderings of the float32 values"""
    num = lambda v: " ".join("%.17g" % float(np.float32(x)) for x in (v if isinstance(v, (tuple, list)) else [v]))  # noqa: E731
    lines = []
    for k, sh in enumerate(scene):
        if sh[-1] is None:
            mat = "none"
        else:
            mat = os.path.join(tmp, "%s_mat%d.bin" % (tag, k))
            O.materials(sh[-1]).tofile(mat)
        if sh[0] == "sphere":
            lines.append("sphere %s %s %s" % (num(sh[1]), num(sh[2]), mat))
        elif sh[0] == "plane":
            lines.append("plane %s %s %s" % (num(sh[1]), num(sh[2]), mat))
        elif sh[0] == "capsule":
            lines.append("capsule %s %s %s %s" % (num(sh[1]), num(sh[2]), num(sh[3]), mat))
        elif sh[0] == "triangle":
            lines.append("triangle %s %s %s %s" % (num(sh[1]), num(sh[2]), num(sh[3]), mat))
        else:
            lines.append("mesh %s %s" % (obj_path(sh[1]), mat))
    path = os.path.join(tmp, tag + ".scene")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return path


def golden_scene_closest(tag, n, tmp, rng, mesh_bounds):
    scene = SC.SCENES[tag]()
    sp = write_scene_file(scene, tmp, tag)
    rays = make_rays(SC.scene_bounds(scene, mesh_bounds), n, rng)
    rp, hp = os.path.join(tmp, "rays.bin"), os.path.join(tmp, "hits.bin")
    rays.tofile(rp)
    run(["closest", sp, rp, len(rays), hp])
    r = np.fromfile(hp, np.float32).reshape(-1, 13)
    np.savez_compressed(os.path.join(OUT, "sceneclosest_%s.npz" % tag), scene=tag, rays=rays, hit=r[:, :11].copy(),
                        shape=r[:, 11].copy().view(np.int32))


def golden_edges(tmp):
    """scene "edges" under make_edge_rays' rays (a generator of its own: no other fixture's draw moves)"""
    scene = SC.SCENES["edges"]()
    sp = write_scene_file(scene, tmp, "edges")
    rays, family, target = make_edge_rays(scene, np.random.default_rng(20261021))
    assert len(rays) <= 4000
    rp, hp = os.path.join(tmp, "edge_rays.bin"), os.path.join(tmp, "edge_hits.bin")
    rays.tofile(rp)
    run(["closest", sp, rp, len(rays), hp])
    r = np.fromfile(hp, np.float32).reshape(-1, 13)
    np.savez_compressed(os.path.join(OUT, "sceneclosest_edges.npz"), scene="edges", rays=rays, hit=r[:, :11].copy(),
                        shape=r[:, 11].copy().view(np.int32), family=family, target=target)


# ---- textures of awkward shapes: tests/golden/oddtex/ (a quad per material) and texsample_oddtex_m{k}.npz ----
ODDTEX = ((1, 1, 3), (1, 9, 4), (7, 1, 3), (5, 3, 4), (33, 17, 3))                          # width, height, channels of material k's texture
ODDTEX_UV = ((0, 0, 1, 1), (-0.5, 0, 1.5, 1), (0, -1, 1, 2), (-1, -1, 2, 2), (0.25, 0, 3, 1))   # u0, v0, u1, v1 over material k's quad
ODDTEX_CENTRES = ((-2.2, 1.2), (0.0, 1.2), (2.2, 1.2), (-1.1, -1.2), (1.1, -1.2))


def oddtex_texels(k):
    """(h, w, channels) uint8: every texel of the texture differs from every other, and so does every alpha"""
    w, h, c = ODDTEX[k]
    rng = np.random.default_rng(7000 + k)
    while True:
        px = rng.integers(0, 256, (h, w, c)).astype(np.uint8)
        if c == 4:
            px[:, :, 3] = rng.choice(256, h * w, replace=False).reshape(h, w)
        if len(np.unique(px[:, :, :3].reshape(-1, 3), axis=0)) == h * w:
            return px


def oddtex_uv(k, rng):
    """about 300 uv pairs for material k: every texel column and row with the neighbouring floats on either side, wrap-around edges"""
    w, h, _ = ODDTEX[k]
    f = np.float32
    edge = np.array([[0, 0], [1, 1], [0.5, 0.5], [-1e-9, 0.25], [0.25, -1e-9], [1.0, 0.0], [0.999999, 0.999999],
                     [2.0, -3.0], [1 / 511.0, 2 / 511.0], [255 / 255.0, 17 / 255.0]], f)

    def grid(n):
        if n == 1:
            return [f(0), f(0.5), f(1)]
        at = [f(i) / f(n - 1) for i in range(n)]
        return [x for a in at for x in (np.nextafter(a, f(-1)), a, np.nextafter(a, f(2)))]
    U, V = grid(w), grid(h)
    pairs = [(U[i], V[(i * 7 + 3) % len(V)]) for i in range(len(U))] + [(U[(i * 5 + 1) % len(U)], V[i]) for i in range(len(V))]
    special = [f(1e-9), f(-1e-9), f(-0.0), f(-1), f(-2), f(-3), f(1 - 2.0 ** -24), f(8388607.5), f(1e9), f(-1e9), f(0), f(1)]
    pairs += [p for s in special for p in ((s, f(0.3)), (f(0.3), s), (s, s))]
    uv = np.concatenate([edge, np.array(pairs, f)])
    return np.concatenate([uv, rng.uniform(-2.5, 2.5, (max(0, 300 - len(uv)), 2)).astype(f)])


def golden_oddtex(tmp):
    """Writes tests/golden/oddtex/ (oddtex.obj, oddtex.mtl, t{k}.png) and, through the reference's own loader and sampler,
    texsample_oddtex_m{k}.npz.  RGB files by the reference's PNG writer (harness `savepng`), RGBA files (it writes no alpha) by Pillow."""
    from PIL import Image
    d = os.path.join(OUT, "oddtex")
    os.makedirs(d, exist_ok=True)
    obj, mtl = ["# a quad per material, facing +z (tilted: a triangle in a z = const plane has a box no ray enters)", "mtllib oddtex.mtl", "vn 0 0 1"], []
    for k, ((w, h, c), (u0, v0, u1, v1), (cx, cy)) in enumerate(zip(ODDTEX, ODDTEX_UV, ODDTEX_CENTRES)):
        px = oddtex_texels(k)
        path = os.path.join(d, "t%d.png" % k)
        if c == 3:
            argb = (np.uint32(255) << 24) | (px[:, :, 0].astype(np.uint32) << 16) | (px[:, :, 1].astype(np.uint32) << 8) | px[:, :, 2]
            ap = os.path.join(tmp, "t%d.argb" % k)
            argb.astype(np.uint32).tofile(ap)
            run(["savepng", ap, w, h, path])
        else:
            Image.fromarray(px, "RGBA").save(path, optimize=False)
        assert (np.asarray(Image.open(path)) == px).all()
        corners = [(cx - 0.9, cy - 0.9, u0, v0), (cx + 0.9, cy - 0.9, u1, v0), (cx + 0.9, cy + 0.9, u1, v1), (cx - 0.9, cy + 0.9, u0, v1)]
        for x, y, u, v in corners:
            obj.append("v %g %g %g" % (x, y, 0.15 * x + 0.1 * y))
        for x, y, u, v in corners:
            obj.append("vt %g %g" % (u, v))
        obj.append("usemtl m%d" % k)
        obj.append("f " + " ".join("%d/%d/1" % (4 * k + i + 1, 4 * k + i + 1) for i in range(4)))
        mtl += ["newmtl m%d" % k, "map_Kd t%d.png" % k, ""]
    open(os.path.join(d, "oddtex.obj"), "w").write("\n".join(obj) + "\n")
    open(os.path.join(d, "oddtex.mtl"), "w").write("\n".join(mtl))
    rng = np.random.default_rng(20261022)
    fed = O.Scene()
    sh = fed.add_mesh_obj(os.path.join(d, "oddtex.obj"), load_textures=False)
    for k in range(len(ODDTEX)):
        uv = oddtex_uv(k, rng)
        up, op = os.path.join(tmp, "uv.bin"), os.path.join(tmp, "tex.bin")
        uv.tofile(up)
        run(["texsample", os.path.join(d, "oddtex.obj"), k, up, len(uv), op])
        rgba = np.fromfile(op, np.float32).reshape(-1, 4)
        fed.set_texture(sh, k, oddtex_texels(k))        # the reference's loader read what was written: its samples are those of the texel array
        assert (fed.texture_sample(sh, k, uv).view(np.uint32) == rgba.view(np.uint32)).all(), k
        np.savez_compressed(os.path.join(OUT, "texsample_oddtex_m%d.npz" % k), uv=uv, material=np.int32(k), rgba=rgba)


def golden_scene_frame(name, tag, W, Hh, ns, depth, preview, seed, pass0, npass, tmp):
    sp, fp = write_scene_file(SC.SCENES[tag](), tmp, tag), os.path.join(tmp, "frame")
    run(["frame", sp, "-", W, Hh, ns, depth, preview, seed, pass0, npass, 0, W * Hh - 1, fp])
    np.savez_compressed(os.path.join(OUT, "sceneframe_%s.npz" % name), scene=tag,
                        params=np.array([W, Hh, ns, depth, preview, seed, pass0, npass], np.int64),
                        accum=np.fromfile(fp + ".accum.f32", np.float32).reshape(-1, 4),
                        argb=np.fromfile(fp + ".argb.u32", np.uint32))


def golden_materials(tmp):
    """The material trees of tests/material_support.py marked `ref`, through the reference's own BounceViewRay / PreviewColor: per tree
    matedge_<name>.npz with a `raytrace` record (TorusKnot, depth 6, the rays and keys of matedge_rays.npz, which all trees share), a 48 x 27 frame
    (2 sub-samples, depth 5, one pass) and the same frame in the preview version; scene "matedge" (three Combine trees on analytic shapes); and the
    depth-16 frames.  A generator of its own: no other fixture's draw moves."""
    import material_support as MS
    rng = np.random.default_rng(20261023)
    bounds = np.load(os.path.join(OUT, "mesh_%s.npz" % MS.MESH))["shape_bounds"]
    rays = make_rays(bounds, 134, rng)
    depth, seed, RW, RH = 6, 4242, 1920, 1080
    keys = np.c_[rng.integers(0, RW * RH, len(rays)), rng.integers(0, 8, len(rays))].astype(np.uint32)
    np.savez_compressed(os.path.join(OUT, "matedge_rays.npz"), mesh=MS.MESH, rays=rays, keys=keys, params=np.array([depth, seed, RW, RH], np.int64))
    mp, rp, kp, op, fp = [os.path.join(tmp, f) for f in ("mat.bin", "rays.bin", "keys.bin", "rt.bin", "frame")]
    rays.tofile(rp)
    keys.tofile(kp)
    W, Hh, ns, fdepth = MS.FRAME
    for name in MS.REF_TREES:
        arr = O.materials(MS.TREES[name][0])
        arr.tofile(mp)
        run(["raytrace", obj_path(MS.MESH), mp, rp, kp, len(rays), depth, 0, seed, RW, RH, op])
        rgb = np.fromfile(op, np.float32).reshape(-1, 3)
        run(["frame", obj_path(MS.MESH), mp, W, Hh, ns, fdepth, 0, MS.SEED, 0, 1, 0, W * Hh - 1, fp])
        accum, argb = np.fromfile(fp + ".accum.f32", np.float32).reshape(-1, 4), np.fromfile(fp + ".argb.u32", np.uint32)
        run(["frame", obj_path(MS.MESH), mp, W, Hh, ns, fdepth, 1, MS.SEED, 0, 1, 0, W * Hh - 1, fp])
        np.savez_compressed(os.path.join(OUT, "matedge_%s.npz" % name), mesh=MS.MESH, material=arr, rgb=rgb,
                            params=np.array([W, Hh, ns, fdepth, 0, MS.SEED, 0, 1], np.int64), accum=accum, argb=argb,
                            preview_argb=np.fromfile(fp + ".argb.u32", np.uint32))
    golden_scene_frame("matedge_d5", "matedge", 64, 36, 2, 5, 0, MS.SEED, 0, 1, tmp)
    golden_scene_frame("matedge_preview", "matedge", 64, 36, 2, 5, 1, MS.SEED, 0, 1, tmp)
    golden_depth16(tmp)


def golden_depth16(tmp):
    """depth 16 = RTW_MAX_BOUNCE: the mirror (its paths end long before: fewer than 8 levels on this mesh), and MS.DEPTH16_TREE, a
    combine(Emissive, Diffuse) whose surviving ray is the incoming one, so that every path that hits the mesh runs to the last level"""
    import material_support as MS
    d16 = MS.DEPTH16
    golden_frame("torus_mirror_d16", d16["mesh"], "mirror", d16["W"], d16["H"], d16["ns"], d16["depth"], 0, d16["seed"], 0, 1, tmp)
    assert MATERIALS["combine_d16"] == MS.DEPTH16_TREE
    golden_frame("torus_combine_d16", d16["mesh"], "combine_d16", d16["W"], d16["H"], d16["ns"], d16["depth"], 0, d16["seed"], 0, 1, tmp)


def main_scenes(tmp, rng, bounds):
    """multi-shape scenes: RSphere / RPlane / RCapsule beside meshes (tests/scenes.py)"""
    for tag in ("default_nofuzz", "quirk", "shapes", "room", "tris"):
        golden_scene_closest(tag, 700, tmp, rng, bounds)
    S = golden_scene_frame
    S("default_d5", "default", 80, 80, 4, 5, 0, 12345, 0, 1, tmp)
    S("default_nofuzz_d5", "default_nofuzz", 80, 80, 4, 5, 0, 12345, 0, 2, tmp)
    S("default_preview", "default", 80, 80, 4, 5, 1, 12345, 0, 1, tmp)
    S("quirk_d4", "quirk", 96, 96, 4, 4, 0, 77, 0, 1, tmp)
    S("quirk_preview", "quirk", 96, 96, 4, 4, 1, 77, 0, 1, tmp)
    S("shapes_d6", "shapes", 96, 64, 4, 6, 0, 9, 1, 2, tmp)
    S("shapes_1spp_d2", "shapes", 50, 70, 1, 2, 0, 9, 0, 1, tmp)
    S("room_d8", "room", 64, 64, 4, 8, 0, 21, 0, 1, tmp)
    S("tris_d5", "tris", 96, 96, 4, 5, 0, 4, 0, 1, tmp)


def main():
    O.build()
    if not os.path.exists(H):
        sys.exit("oracle/_ref/ref_harness is not built (no /root/reference here?)")
    rng = np.random.default_rng(20261004)
    if "--worker-only" in sys.argv:        # add the ThreadWorker_Render fixtures without regenerating the others
        with tempfile.TemporaryDirectory() as tmp:
            main_worker(tmp)
        return
    if "--misc-only" in sys.argv:
        with tempfile.TemporaryDirectory() as tmp:
            golden_misc(tmp)
        return
    if "--edges-only" in sys.argv:         # add the edge-case fixtures (tests/test_edges_*.py) without regenerating the others
        with tempfile.TemporaryDirectory() as tmp:
            golden_edges(tmp)
            golden_oddtex(tmp)
        return
    if "--scenes-only" in sys.argv:        # add the multi-shape fixtures without regenerating the others
        rng = np.random.default_rng(20261005)
        with tempfile.TemporaryDirectory() as tmp:
            bounds = {n: np.load(os.path.join(OUT, "mesh_%s.npz" % n))["shape_bounds"] for n in ("TorusKnot", "BlenderMonkey", "unitychan")}
            main_scenes(tmp, rng, bounds)
        return
    if "--materials-only" in sys.argv:     # add the material-tree fixtures (tests/test_material_*.py) without regenerating the others
        with tempfile.TemporaryDirectory() as tmp:
            golden_materials(tmp)
        return
    with tempfile.TemporaryDirectory() as tmp:
        bounds = {}
        for name in ("TorusKnot", "BlenderMonkey", "unitychan"):
            bounds[name] = golden_mesh(name, tmp)
            golden_closest(name, bounds[name], 600 if name == "unitychan" else 900, tmp, rng)
        golden_texsample("unitychan", 4, 600, tmp, rng)     # 256x256 RGBA (cheek)
        golden_texsample("unitychan", 0, 600, tmp, rng)     # 512x512 RGB (skin)
        F = golden_frame
        F("torus_diffuse_4spp_d4", "TorusKnot", "diffuse", 64, 64, 4, 4, 0, 12345, 0, 1, tmp)
        F("torus_diffuse_1spp_d1", "TorusKnot", "diffuse", 64, 48, 1, 1, 0, 7, 0, 1, tmp)
        F("torus_diffuse_3pass_d10", "TorusKnot", "diffuse", 64, 64, 4, 10, 0, 12345, 0, 3, tmp)
        F("torus_preview", "TorusKnot", "diffuse", 64, 64, 4, 4, 1, 12345, 0, 1, tmp)
        F("torus_mirror_d6", "TorusKnot", "mirror", 64, 64, 4, 6, 0, 99, 0, 1, tmp)
        F("torus_blendfuzz_d6", "TorusKnot", "blendfuzz", 64, 64, 4, 6, 0, 99, 0, 1, tmp)
        F("monkey_blendfuzz_d6", "BlenderMonkey", "blendfuzz", 96, 54, 4, 6, 0, 5, 1, 2, tmp)
        F("torus_checker", "TorusKnot", "checker", 64, 64, 2, 4, 0, 3, 0, 1, tmp)
        F("torus_checker_preview", "TorusKnot", "checker", 64, 64, 4, 4, 1, 3, 0, 1, tmp)
        F("torus_combine", "TorusKnot", "combine", 64, 64, 4, 5, 0, 3, 0, 1, tmp)
        F("torus_null", "TorusKnot", "null", 64, 64, 4, 5, 0, 3, 0, 1, tmp)
        F("torus_partial_albedo", "TorusKnot", "partial", 64, 64, 4, 5, 0, 3, 0, 1, tmp)
        F("unitychan_diffuse_d4", "unitychan", "diffuse", 96, 96, 4, 4, 0, 12345, 0, 1, tmp)
        F("unitychan_preview", "unitychan", "diffuse", 96, 96, 4, 4, 1, 12345, 0, 1, tmp)
        golden_raytrace("unitychan_diffuse", "unitychan", "diffuse", 500, 6, 4242, 1920, 1080, tmp, rng, bounds["unitychan"])
        golden_raytrace("monkey_blendfuzz", "BlenderMonkey", "blendfuzz", 900, 6, 4242, 1920, 1080, tmp, rng, bounds["BlenderMonkey"])
        main_scenes(tmp, np.random.default_rng(20261005), bounds)
        main_worker(tmp)
        golden_misc(tmp)
        golden_edges(tmp)
        golden_oddtex(tmp)
        golden_materials(tmp)
    total = sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT) if f.endswith(".npz"))
    print("golden fixtures written: %.2f MB" % (total / 1e6))


if __name__ == "__main__":
    main()
