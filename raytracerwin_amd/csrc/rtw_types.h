// rtw_types.h -- plain-data layouts shared by the host scene builder and the HIP kernels.
//
// HBM layout (per committed scene; everything read-only while rendering):
//   nodes   RtwNode[2T-1]   32 B   preorder, left child = i+1, `skip` = next node after the subtree
//   tris    RtwTri[T]       64 B   leaf order: 3 positions + face normal + plane offset + original index
//   shade   RtwShade[T]     64 B   leaf order: 3 vertex normals, 3 uv pairs, material id
//   texels  uint32[...]     RGBA8 atlas, one slab per texture; linearised through a 256-entry LUT
//   unit    float[3*0xFFFFFF]  the reference's pseudo-random unit-vector table (per context)
#pragma once
#include <stdint.h>

struct RtwNode {            // 2 x 16 B
    float min_x, min_y, min_z; int32_t skip;
    float max_x, max_y, max_z; int32_t tri;      // leaf slot, or -1 for an internal node
};
static_assert(sizeof(RtwNode) == 32, "RtwNode");

struct RtwPNode {           // 2 x 16 B
    float min_x, max_x, min_y, max_y;
    float min_z, max_z; int32_t skip; int32_t link;   // link >= 0: a leaf's slot; < 0: internal, left child = record -1 - link
};
static_assert(sizeof(RtwPNode) == 32, "RtwPNode");

struct RtwTri {             // 4 x 16 B
    float p0x, p0y, p0z, nx;
    float p1x, p1y, p1z, ny;
    float p2x, p2y, p2z, nz;
    float d1; int32_t orig; int32_t pad0, pad1;  // d1 = dot(N, p0); orig = triangle index in the mesh
};
static_assert(sizeof(RtwTri) == 64, "RtwTri");

struct RtwShade {           // 4 x 16 B
    float n0x, n0y, n0z, n1x;
    float n1y, n1z, n2x, n2y;
    float n2z, u0, v0, u1;
    float v1, u2, v2; int32_t material;
};
static_assert(sizeof(RtwShade) == 64, "RtwShade");

struct RtwTexture {         // 16 B
    uint32_t offset;        // first texel in the atlas
    int32_t width, height;
    int32_t valid;
};

struct RtwMaterialNode {    // mirrors rtw_material_node
    int32_t type; float r, g, b; float param; int32_t child_a, child_b; int32_t pad;
};

#define RTW_DEV_MAX_TEXTURES 64
#define RTW_DEV_MAX_MATERIAL_NODES 64
#define RTW_DEV_MAX_SHAPES 32
#define RTW_SHAPE_MESH 0
#define RTW_SHAPE_SPHERE 1
#define RTW_SHAPE_PLANE 2
#define RTW_SHAPE_CAPSULE 3
#define RTW_SHAPE_TRIANGLE 4

struct RtwShapeDev {
    const RtwNode* nodes;
    const RtwTri* tris;
    const RtwShade* shade;
    const uint32_t* texels;
    // flat hierarchy over the leaves in preorder (16 consecutive entries of a level share one entry of the next):
    // level 0 = the leaves' own boxes, 1 = groups of 16 leaves, 2 = groups of 256.  Entry i of a level is the 24 bytes
    // flat[l][6 i ..]: (min x, max x), (min y, max y), (min z, max z) -- one pair per axis, so that (pair - origin) * reciprocal
    // is one packed subtract and one packed multiply; flat_pad[l] entries are allocated (whole waves may read past flat_n[l]).
    const float* flat[3];
    int32_t flat_n[3], flat_pad[3];
    // the same binary tree once more for the ray-per-lane walk (gtrace_kernel): RtwNode records with EXPLICIT links -- `skip` as in
    // `nodes`, `tri` >= 0 a leaf's slot, < 0 an internal node whose left child is record -1 - tri -- stored so that the tnodes_top
    // records of the tree's upper levels come first, in preorder (a block stages them in LDS), followed by the subtrees below them,
    // each contiguous in preorder.  The walk visits the records in the reference's order whatever their place in memory.
    // A record is RtwPNode: the box as (min, max) PAIRS per axis, so that (pair - origin) * reciprocal is one packed subtract and one
    // packed multiply per axis (v_pk_add_f32 / v_pk_mul_f32: component-wise the reference's float operations).
    const struct RtwPNode* tnodes;
    const float* planes;            // per leaf slot 4 floats: the triangle's face normal and plane offset (RtwTri nx, ny, nz, d1) on their own, 16 bytes a leaf: the
                                    // ray-per-lane walk drops a leaf whose triangle faces away from the ray's origin (RRay::TestIntersectionWithTriangle's first
                                    // rejection, Src/RRay.cpp:156-158, which does not depend on the segment) before it is ever noted; null: not built
    float bmin[3], bmax[3];         // RShape::Aabb (all `v` lines)
    int32_t n_nodes, n_tris;
    int32_t n_textures;             // size of the reference's Textures vector (= triangle count when an MTL exists)
    int32_t has_material;
    int32_t n_material_nodes;
    // RTW_SHAPE_MESH: everything above; a sphere / plane / capsule has no arrays, only these (Src/Shapes.h:46-112):
    //   sphere: pa = Center, radius;  plane: pa = Normal, pb = Point;  capsule: pa = Start, pb = End, radius;  triangle: see pc
    int32_t kind;
    float pa[3], pb[3], radius;
    float pc[3], pn[3], pd1;        // triangle (RTriangle, Src/Shapes.h:106-130): pa, pb, pc = Points[0..2]; pn = its face normal and pd1 = dot(pn, pa) as
                                    // RRay::TestIntersectionWithTriangle computes them at every test (Src/RRay.cpp:138-145), here once on the host
    int32_t tnodes_top;
    RtwTexture textures[RTW_DEV_MAX_TEXTURES];
    RtwMaterialNode material[RTW_DEV_MAX_MATERIAL_NODES];
};

struct RtwSceneDev {
    int32_t n_shapes;
    int32_t prune;
    int32_t traversal;              // 1 (default): bins, flat hierarchy and link tree may be used; 0: binary preorder walk only (reference visit counts)
    int32_t debug_table_mask;       // timing experiments only: nonzero -> unit-table index &= mask (changes the image)
    const float* unit_table;        // 3 floats per entry
    const float* gamma_thr;         // 256
    const float* texel_lut;         // 256
    unsigned long long* stats;      // 8 counters or nullptr
    RtwShapeDev shapes[RTW_DEV_MAX_SHAPES];
};

// The camera (rtw_camera of rtwin.h): pixel (x, y), sub-sample offset (ox, oy) looks along
//   v[k] = (right[k] * (dx + ox) + up[k] * (dy + oy)) + forward[k] * focal,   dir = normalized(v),   origin = eye
// with dx, dy as the reference computes them (Src/RayTracerProgram.cpp:141-142).  The reference's own camera is
// eye (0, 0, 7), right (1, 0, 0), up (0, 1, 0), forward (0, 0, -1), focal 0.5.
struct RtwCamera { float eye[3], right[3], up[3], forward[3]; float focal; };
static_assert(sizeof(RtwCamera) == 52, "RtwCamera");
inline RtwCamera rtw_default_camera()
{
    const RtwCamera c = { { 0.0f, 0.0f, 7.0f }, { 1.0f, 0.0f, 0.0f }, { 0.0f, 1.0f, 0.0f }, { 0.0f, 0.0f, -1.0f }, 0.5f };
    return c;
}

// What the screen-bin routine (rtw_shared.h bins_of_leaf, run by scene_host.cpp build_bins and by rtw_build_kernels.h bins_pass_kernel) needs
// of a camera, in double: computed once on the host by rtw_bins_camera() and handed to either side.
struct RtwBinsCam {
    double eye[3], right[3], up[3], forward[3];
    double k;                       // 2 * focal * height: a point q (relative to the eye) is seen at x = W/2 - k (q.right) / (q.forward)
    double margin;                  // pixels a leaf's projection is grown by (below)
    float eye_f[3];                 // the eye as the kernels' rays carry it (the facing test is the reference's float test)
    int32_t ok;                     // 0: this camera gets no bins at all
};
// The margin.  (1) Jitter: a sub-sample looks through a point up to 1.25 / (4 W) off its pixel centre in dx and dy
// (Src/RayTracerProgram.cpp:147-162), i.e. 1.25 H / (2 W) pixels; plus one pixel of slack.  (2) A basis that is orthonormal only to
// rounding.  With a = dx + ox, b = dy + oy, f = focal a ray's direction is v = a R + b U + f F and a point on it q = t v, so the builders see
//   q.R = t (a R.R + b U.R + f F.R) = t (a + n),     q.F = t (a R.F + b U.F + f F.F) = t (f + d),     |n|, |d| <= e S
// where e = the largest of |R.R - 1|, |U.U - 1|, |F.F - 1|, |R.U|, |R.F|, |U.F| and S = A + B + f, A >= |a|, B >= |b| on the screen
// (A = W / (4 H) + 1.25 / (4 W), B = 1 / 4 + 1.25 / (4 W)).  The projected a' = f (a + n) / (f + d) differs from a by
//   |a' - a| = |f n - a d| / |f + d| <= e S (f + A) / (f - e S) = e S (1 + A / f) / (1 - e S / f)
// (the same for b with B; the larger of A and B is used for both), which is 2 H times as much in pixels.  e is measured in double from the
// struct's floats: exactly 0 for the default camera (whose margin is therefore the fixed camera's), ~1e-7 after rtw_camera_look_at,
// at most ~3e-4 for a basis the validation accepts.  A camera with e S >= f / 2 gets no bins.
inline RtwBinsCam rtw_bins_camera(const RtwCamera& c, int width, int height)
{
    RtwBinsCam b;
    for (int k = 0; k < 3; k++) { b.eye[k] = c.eye[k]; b.right[k] = c.right[k]; b.up[k] = c.up[k]; b.forward[k] = c.forward[k]; b.eye_f[k] = c.eye[k]; }
    const double f = (double)c.focal, W = (double)width, H = (double)height;
    b.k = 2.0 * f * H;
    auto dot = [](const double* u, const double* v) { return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]; };
    auto ab = [](double x) { return x < 0 ? -x : x; };
    double e = ab(dot(b.right, b.right) - 1.0);
    const double o[5] = { ab(dot(b.up, b.up) - 1.0), ab(dot(b.forward, b.forward) - 1.0), ab(dot(b.right, b.up)), ab(dot(b.right, b.forward)), ab(dot(b.up, b.forward)) };
    for (int i = 0; i < 5; i++) if (o[i] > e) e = o[i];
    const double A = W / (4.0 * H) + 1.25 / (4.0 * W), B = 0.25 + 1.25 / (4.0 * W), M = A > B ? A : B, S = A + B + f;
    b.ok = (f > 0 && e == e && e * S < 0.5 * f) ? 1 : 0;
    b.margin = 1.0 + 1.25 * H / (2.0 * W);
    if (b.ok && e > 0) b.margin += 2.0 * H * (e * S * (1.0 + M / f) / (1.0 - e * S / f));
    return b;
}

struct RtwRenderParams {
    int32_t width, height;
    int32_t begin, count;           // linear work items: pixel = map(begin + i)
    int32_t task_rows, rank, world; // world <= 1: contiguous range
    int32_t max_bounce, preview, pass_index, sub_samples;
    uint32_t seed;
    // tiled work mapping (tile_w != 0): wave w of the launch renders the tile_w x tile_h pixel tile number w of its rows,
    // aligned to the screen's bin grid; `bins` then holds, per shape, the leaves whose box can be met by a camera ray of each bin
    int32_t tile_w, tile_h, tile_shift, tiles_per_row;
    int32_t row0, nrows;            // contiguous range: first screen row and number of rows; task partition: number of virtual rows
    int32_t lead_shapes;            // the scene's first lead_shapes shapes are spheres / planes / capsules / triangles;
                                    // the lane that sets up a path's next segment (shade_hit_step) tests them there, one ray per lane, and
                                    // leaves the partial scene query in the path's hit record; the wave-per-ray trace continues from it
    int32_t n_jobs;                 // entries of tile_order
    const struct RtwBinsDev* bins;  // [n_shapes] or null
    const uint32_t* tile_order;     // full-frame launches: the order in which the primary kernel takes the tiles (null = as numbered)
    const float* cam_dx;            // tiled mapping: dx of every pixel column / dy of every pixel row (Src/RayTracerProgram.cpp:141-142),
    const float* cam_dy;            // computed once on the host with the same float operations
    RtwCamera cam;                  // the scene's camera, by value (wave-uniform: scalar registers)
    int32_t cam_general;            // 0: cam is the default camera bit for bit -> the kernels' fixed-pose instantiations (constants instead of cam); 1: the general ones
    // the thin lens (rtw_lens of rtwin.h), a launch parameter like the camera.  lens != 0 (aperture_radius > 0): every camera ray has its own origin on
    // the aperture disc -> the kernels' LENS instantiations (which imply the general camera), no screen bins, every tile busy
    int32_t lens;
    float lens_radius, lens_focus;
};
// the lens point's random stream: stream_key(seed, pixel, (pass * 4 + sub) | RTW_LENS_STREAM), beside the path's own (whose counter the lens never moves)
#define RTW_LENS_STREAM 0x80000000u

// screen-space bins of one shape for one (width, height, tile shape): CSR over the bins, entries = node index of a leaf, ascending
struct RtwBinsDev {
    const uint32_t* off;            // n_bins + 1 offsets, or null: no bins for this shape (camera too close to it) -> tree walk
    const uint32_t* ent;
};

// ---- pass-batched pipeline (pipeline 4): the passes first_pass .. first_pass + n_passes - 1 of one rtw_render_passes call share one
// set of launches.  Tiles of the launch are either BUSY (some shape lists a leaf in the tile's bin, or has no bins) or SKY-ONLY.
// A path's slot = ((b * sub_samples + sub) * n_passes + k) * 64 + lane   (b = rank of its tile in the busy list, k = pass - first_pass).
struct RtwGroupParams {
    RtwRenderParams rp;             // frame, tile mapping, bounce limit, seed, bins, camera tables (pass_index unused)
    int32_t first_pass, n_passes;
    int32_t n_busy, n_sky, n_jobs;
    const uint32_t* busy_tiles;     // tile numbers of the busy tiles, heaviest bins first; null: tile = first_tile + b (every tile of the range)
    const uint32_t* sky_tiles;      // tile numbers of the sky-only tiles
    const uint32_t* jobs;           // primary kernel: b | (sub-sample + 1) << 24 (0 in bits 24..27: every sub-sample); null: job = b
    int32_t range_begin, range_end; // inclusive pixel range that is rendered (a lane outside it is dead)
    int32_t first_tile;
    int32_t primary_passes;         // passes one wave of the primary kernel takes for its tile (> 1: x sub-samples <= 4; -1: one ray set at a time, no shared walk)
};

// random-stream constants (shared with the oracle by specification, not by code)
#define RTW_TABLE_SIZE 0xFFFFFFu
#define RTW_TABLE_STRIDE 16u
#define RTW_TABLE_SEED 0x52544142u
