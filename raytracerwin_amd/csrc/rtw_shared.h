// rtw_shared.h -- the arithmetic the host library and the HIP kernels both compute, written once: the random stream, the camera
// and lens rays, the records derived from a tree, and the screen bins of a leaf.  Plain functions of plain values; the host and the
// kernels call the same text, so the two sides agree by construction.
//
// Every float expression keeps the reference's operand order (build with -ffp-contract=off, correctly rounded divide / sqrt).
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "rtw_types.h"

#if defined(__HIP__)
#define RTW_HD __host__ __device__ __forceinline__
#else
#define RTW_HD inline
#endif

// ---- float3 -----------------------------------------------------------------------------------------------------------------
struct f3 { float x, y, z; };
RTW_HD f3 mk(float x, float y, float z) { f3 r; r.x = x; r.y = y; r.z = z; return r; }
RTW_HD f3 operator+(f3 a, f3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
RTW_HD f3 operator-(f3 a, f3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
RTW_HD float dot(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
RTW_HD f3 cross(f3 a, f3 b) { return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
RTW_HD bool near_zero(float a) { return fabsf(a) < FLT_EPSILON; }   // FLT_EQUAL_ZERO, Src/MathHelper.h:12
// RVec3::GetNormalizedVec3 (Src/RVector.h:169-183): tiny vectors are returned un-normalised
RTW_HD f3 normalized(f3 v)
{
    float sq = v.x * v.x + v.y * v.y + v.z * v.z;
    if (!near_zero(sq)) { float inv = 1.0f / sqrtf(sq); v.x *= inv; v.y *= inv; v.z *= inv; }
    return v;
}

// ---- random stream (specification shared with the oracle) ----------------------------------------------------------------------
RTW_HD uint32_t mix32(uint32_t x) { x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16; return x; }
RTW_HD uint32_t stream_key(uint32_t seed, uint32_t pixel, uint32_t sample)
{
    uint32_t h = mix32(seed ^ 0x9E3779B9u);
    h = mix32(h + pixel);
    return mix32(h + sample);
}
RTW_HD uint32_t stream_draw31(uint32_t key, uint32_t counter) { return mix32(key + counter) >> 1; }    // the stream's rand()
// RMath::Random (Src/Math.h:17-20), (float)rand() / RAND_MAX, of draw `counter` of the stream `key`
RTW_HD float stream_uniform(uint32_t key, uint32_t counter) { return (float)(int32_t)stream_draw31(key, counter) / 2147483648.0f; }
RTW_HD uint32_t table_phase(uint32_t seed) { return mix32(seed ^ 0x7AB1E5u) % RTW_TABLE_SIZE; }   // 32-bit: fine

// ---- camera ray (Src/RayTracerProgram.cpp:141-165; rtw_types.h RtwCamera) ------------------------------------------------------
RTW_HD float frame_aspect(int width, int height) { return (float)width / (float)height; }
RTW_HD float pixel_dx(int x, int width, float aspect) { return -(float)(x - width / 2) / (width * 2) * aspect; }
RTW_HD float pixel_dy(int y, int height) { return -(float)(y - height / 2) / (height * 2); }
// Sub-sample i looks through (dx + ox, dy + oy): its place in the pixel's 2 x 2 grid, then moved by a jitter of width offset_radius,
// ox = jittered(ox, u1, offset_radius), oy = jittered(oy, u2, offset_radius) with u1, u2 the first two draws of the path's stream
RTW_HD void sample_grid(int width, int i, float& ox, float& oy, float& offset_radius)
{
    const float inv_pixel_radius = 1.0f / (width * 4);
    offset_radius = inv_pixel_radius * 0.5f;
    ox = (i & 1) ? inv_pixel_radius : 0.0f;
    oy = (i & 2) ? inv_pixel_radius : 0.0f;
}
RTW_HD float jittered(float o, float u, float offset_radius) { return o + (u - 0.5f) * offset_radius; }
// v of rtw_types.h RtwCamera, before it is normalised: every product and every sum rounded on its own
RTW_HD f3 camera_view(const RtwCamera& c, float a, float b)
{
    return mk((c.right[0] * a + c.up[0] * b) + c.forward[0] * c.focal,
              (c.right[1] * a + c.up[1] * b) + c.forward[1] * c.focal,
              (c.right[2] * a + c.up[2] * b) + c.forward[2] * c.focal);
}

// ---- the thin lens (rtw_lens of rtwin.h) ----------------------------------------------------------------------------------------
// The point on the unit disc: rejection sampling, at most eight tries, from a stream of its own -- key_l = stream_key(seed, pixel,
// (pass * 4 + sub) | RTW_LENS_STREAM), try t reads counters 2 t and 2 t + 1 -- so the path's own stream stands at counter 2 after the camera
// ray with or without a lens.  No try inside the disc (4.5e-6 of the samples): the centre.
RTW_HD void lens_point(uint32_t key_l, float& lx, float& ly)
{
    lx = 0.0f; ly = 0.0f;
    for (uint32_t t = 0; t < 8u; t++) {
        const float x = 2.0f * stream_uniform(key_l, 2u * t) - 1.0f, y = 2.0f * stream_uniform(key_l, 2u * t + 1u) - 1.0f;
        if (x * x + y * y <= 1.0f) { lx = x; ly = y; break; }
    }
}
// The ray through the point `focus` along `forward` that the pinhole ray of view vector v meets, from the lens point (lx, ly) of an aperture
// of radius `radius`: every product and every sum rounded on its own (include/rtwin.h spells the steps out; the tests' NumPy model repeats them).
RTW_HD void lens_ray(const RtwCamera& c, const float& radius, const float& focus, f3 v, float lx, float ly, f3& origin, f3& dir)
{
    const float s = focus / c.focal;
    const float lxr = lx * radius, lyr = ly * radius;
    const f3 off = mk(c.right[0] * lxr + c.up[0] * lyr, c.right[1] * lxr + c.up[1] * lyr, c.right[2] * lxr + c.up[2] * lyr);
    const f3 w = mk(v.x * s - off.x, v.y * s - off.y, v.z * s - off.z);
    const float inv = 1.0f / sqrtf((w.x * w.x + w.y * w.y) + w.z * w.z);
    origin = mk(c.eye[0] + off.x, c.eye[1] + off.y, c.eye[2] + off.z);
    dir = mk(w.x * inv, w.y * inv, w.z * inv);
}

// ---- records derived from the tree ------------------------------------------------------------------------------------------------
// A leaf's triangle with the face normal RRay::TestIntersectionWithTriangle recomputes at every test (Src/RRay.cpp:138-145:
// normalize(cross(p1 - p0, p2 - p0)), tiny vectors left as they are); it only depends on the triangle
RTW_HD RtwTri tri_record(f3 p0, f3 p1, f3 p2, int32_t orig)
{
    const f3 n = normalized(cross(p1 - p0, p2 - p0));
    RtwTri r;
    r.p0x = p0.x; r.p0y = p0.y; r.p0z = p0.z; r.nx = n.x;
    r.p1x = p1.x; r.p1y = p1.y; r.p1z = p1.z; r.ny = n.y;
    r.p2x = p2.x; r.p2y = p2.y; r.p2z = p2.z; r.nz = n.z;
    r.d1 = dot(n, p0); r.orig = orig; r.pad0 = r.pad1 = 0;
    return r;
}
// the shading inputs RMeshShape::TestRayIntersection gathers per hit (Src/MeshShape.cpp:303-326); a texcoord's z is unused
RTW_HD RtwShade shade_record(f3 n0, f3 n1, f3 n2, f3 t0, f3 t1, f3 t2, int32_t material)
{
    RtwShade s;
    s.n0x = n0.x; s.n0y = n0.y; s.n0z = n0.z; s.n1x = n1.x; s.n1y = n1.y; s.n1z = n1.z; s.n2x = n2.x; s.n2y = n2.y; s.n2z = n2.z;
    s.u0 = t0.x; s.v0 = t0.y; s.u1 = t1.x; s.v1 = t1.y; s.u2 = t2.x; s.v2 = t2.y;
    s.material = material;
    return s;
}
// node i's record of the explicit-link array; place[j] = where node j's record goes (place[n_nodes] = n_nodes)
RTW_HD RtwPNode link_record(const RtwNode& s, const int32_t* place, int i)
{
    RtwPNode t;
    t.min_x = s.min_x; t.max_x = s.max_x; t.min_y = s.min_y; t.max_y = s.max_y; t.min_z = s.min_z; t.max_z = s.max_z;
    t.skip = place[s.skip];
    t.link = s.tri >= 0 ? s.tri : -1 - place[i + 1];
    return t;
}
// flat hierarchy (RtwShapeDev::flat): an entry is six floats, a (min, max) pair per axis.  Level 0: a leaf's own box
RTW_HD void flat_leaf_entry(const RtwNode& s, float* e)
{
    e[0] = s.min_x; e[1] = s.max_x; e[2] = s.min_y; e[3] = s.max_y; e[4] = s.min_z; e[5] = s.max_z;
}
// entry k of level l + 1 (`upper`) = union of the entries [16 k, 16 k + 16) of level l (`lower`, n_lower entries)
RTW_HD void flat_union_entry(const float* __restrict__ lower, int n_lower, float* __restrict__ upper, int k)
{
    float lo[3] = { FLT_MAX, FLT_MAX, FLT_MAX }, hi[3] = { -FLT_MAX, -FLT_MAX, -FLT_MAX };
    for (int i = 16 * k; i < 16 * k + 16 && i < n_lower; i++)
        for (int c = 0; c < 3; c++) {
            const float a = lower[(size_t)i * 6 + 2 * c], b = lower[(size_t)i * 6 + 2 * c + 1];
            if (a < lo[c]) lo[c] = a;
            if (b > hi[c]) hi[c] = b;
        }
    for (int c = 0; c < 3; c++) { upper[(size_t)k * 6 + 2 * c] = lo[c]; upper[(size_t)k * 6 + 2 * c + 1] = hi[c]; }
}

// ---- screen-space bins of the scene's camera (rtw_types.h RtwBinsCam) --------------------------------------------------------------
// Pixel (x, y), sub-sample offset (ox, oy) looks along (dx + ox) right + (dy + oy) up + focal forward, so a point q (relative to the eye,
// depth = q.forward > 0) is seen at x = W/2 - 2 focal H (q.right) / depth, y = H/2 - 2 focal H (q.up) / depth (the offsets move a sample by
// less than half a pixel).  For the reference's own camera -- eye (0, 0, 7), the axes, focal 0.5 -- these are x = W/2 + H q.x / q.z,
// y = H/2 + H q.y / q.z with the same roundings.  A bin lists the leaves whose triangle a camera ray of the bin's pixels could ACCEPT: the
// triangle faces the camera (the reference's own float test, identical for every camera ray) and its projection, grown by `margin` pixels
// (rtw_types.h rtw_bins_camera), touches the bin (separating-axis test against the bin's rectangle).  A leaf left out would have been box- or
// triangle-tested by the reference and rejected, which changes no result; the kernels still run the reference's box and triangle tests on
// every listed leaf, per ray.
//
// A width x height frame cut into bx x by bins of bin_w x bin_h pixels (those at the right / bottom edge may be partial) and its camera
struct RtwBinsGeom { int width, height, bin_w, bin_h, bx, by; double margin; RtwBinsCam cam; };     // margin = cam.margin (rtw_types.h rtw_bins_camera)

// The bins of one leaf: calls f(bin) for every bin the leaf is listed in; returns false when the MESH gets no bins at all.
template <typename F>
RTW_HD bool bins_of_leaf(const RtwNode& nd, const RtwTri& t, const RtwBinsGeom& g, F f)
{
    const double cx = (double)(g.width / 2), cy = (double)(g.height / 2);
    const RtwBinsCam& cam = g.cam;
    for (int c = 0; c < 8; c++) {                           // a corner of the leaf's box not in front of the eye: no bins for this mesh
        const double qx = (double)((c & 1) ? nd.max_x : nd.min_x) - cam.eye[0], qy = (double)((c & 2) ? nd.max_y : nd.min_y) - cam.eye[1],
                     qz = (double)((c & 4) ? nd.max_z : nd.min_z) - cam.eye[2];
        const double depth = qx * cam.forward[0] + qy * cam.forward[1] + qz * cam.forward[2];
        if (!(depth > 0.01)) return false;
    }
    // Every camera ray starts at the eye: the reference's first rejection, "origin behind the triangle's plane"
    // (d2 = N.O - N.P0 < 0, Src/RRay.cpp:156-160), is the same float computation for all of them, so a triangle that
    // fails it is accepted by no camera ray and is listed nowhere.
    {
        const float ox = cam.eye_f[0], oy = cam.eye_f[1], oz = cam.eye_f[2];
        const float d0 = t.nx * ox + t.ny * oy + t.nz * oz;
        const float d2 = d0 - t.d1;
        if (d2 < 0) return true;
    }
    // the triangle's projection (an accepted hit lies inside the triangle, so its pixel lies inside this projection)
    const double vx[3] = { t.p0x, t.p1x, t.p2x }, vy[3] = { t.p0y, t.p1y, t.p2y }, vz[3] = { t.p0z, t.p1z, t.p2z };
    double sx[3], sy[3];
    bool finite = true;
    for (int k = 0; k < 3; k++) {
        const double qx = vx[k] - cam.eye[0], qy = vy[k] - cam.eye[1], qz = vz[k] - cam.eye[2];
        const double depth = qx * cam.forward[0] + qy * cam.forward[1] + qz * cam.forward[2];
        const double qr = qx * cam.right[0] + qy * cam.right[1] + qz * cam.right[2], qu = qx * cam.up[0] + qy * cam.up[1] + qz * cam.up[2];
        sx[k] = cx - cam.k * qr / depth; sy[k] = cy - cam.k * qu / depth;
        finite = finite && sx[k] == sx[k] && sy[k] == sy[k] && fabs(sx[k]) < 1e12 && fabs(sy[k]) < 1e12;
    }
    if (!finite) return false;
    const double xa = fmin(sx[0], fmin(sx[1], sx[2])), xb = fmax(sx[0], fmax(sx[1], sx[2]));
    const double ya = fmin(sy[0], fmin(sy[1], sy[2])), yb = fmax(sy[0], fmax(sy[1], sy[2]));
    double fx0 = floor(xa - g.margin), fx1 = ceil(xb + g.margin), fy0 = floor(ya - g.margin), fy1 = ceil(yb + g.margin);
    if (fx1 < 0 || fy1 < 0 || fx0 > g.width - 1 || fy0 > g.height - 1) return true;      // off screen
    if (fx0 < 0) fx0 = 0;
    if (fy0 < 0) fy0 = 0;
    if (fx1 > g.width - 1) fx1 = g.width - 1;
    if (fy1 > g.height - 1) fy1 = g.height - 1;
    const int bx0 = (int)fx0 / g.bin_w, bx1 = (int)fx1 / g.bin_w, by0 = (int)fy0 / g.bin_h, by1 = (int)fy1 / g.bin_h;
    // edges of the projected triangle with outward normals (skipped when the projection is degenerate)
    const double area2 = (sx[1] - sx[0]) * (sy[2] - sy[0]) - (sx[2] - sx[0]) * (sy[1] - sy[0]);
    const double scale = fabs(xb - xa) + fabs(yb - ya) + 1.0;
    const bool use_edges = fabs(area2) > 1e-9 * scale * scale;
    for (int yb_ = by0; yb_ <= by1; yb_++) {
        for (int xb_ = bx0; xb_ <= bx1; xb_++) {
            bool separated = false;
            if (use_edges) {
                // the bin's pixels, grown by the margin
                const double rx0 = (double)(xb_ * g.bin_w) - g.margin, rx1 = (double)(xb_ * g.bin_w + g.bin_w - 1) + g.margin;
                const double ry0 = (double)(yb_ * g.bin_h) - g.margin, ry1 = (double)(yb_ * g.bin_h + g.bin_h - 1) + g.margin;
                for (int e = 0; e < 3 && !separated; e++) {
                    const int a = e, b2 = (e + 1) % 3, c = (e + 2) % 3;
                    double nx = sy[b2] - sy[a], ny = -(sx[b2] - sx[a]);            // normal of edge a -> b
                    if (nx * (sx[c] - sx[a]) + ny * (sy[c] - sy[a]) > 0) { nx = -nx; ny = -ny; }      // pointing away from the third vertex
                    const double len = sqrt(nx * nx + ny * ny);
                    if (!(len > 0)) continue;
                    // the rectangle's corner that is deepest along -n: if even it is outside, the whole rectangle is
                    const double px = nx > 0 ? rx0 : rx1, py = ny > 0 ? ry0 : ry1;
                    if ((nx * (px - sx[a]) + ny * (py - sy[a])) / len > 1e-6) separated = true;
                }
            }
            if (!separated) f(yb_ * g.bx + xb_);
        }
    }
    return true;
}
