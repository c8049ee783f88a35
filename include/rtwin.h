/*
 * rtwin.h -- C ABI of the MI355X-native ray-trace hot path (librtwin.so).
 *
 * The reference (aosyang/RayTracerWin) has no FFI: its hot path is reached only through
 * in-process C++ calls.  The narrowest seam is the pixel-range task call
 *     void ThreadWorker_Render(int begin, int end, int MaxBounceCount, const RenderOption&)
 * (Src/RayTracerProgram.cpp:131), fed by a scene built with
 *     RayTracerScene::AddShape(RMeshShape::Create(path), material)   (Src/RayTracerScene.cpp:25)
 * and drained through the global accuBuffer[] / bitcolor[] arrays (Src/RayTracerProgram.cpp:49,77).
 * Every entry point below names the reference interface it replaces.  Plain pointers and
 * sizes only; all device memory is owned by the library behind opaque handles (or wrapped
 * from the caller via rtw_framebuffer_wrap).  Every function returns RTW_OK (0) or a
 * negative rtw_status; rtw_last_error() gives the message for the calling thread.
 *
 * There is no CPU fallback: without a HIP device every device entry point fails with
 * RTW_ERR_NO_DEVICE.
 */
#ifndef RTWIN_H
#define RTWIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    RTW_OK = 0,
    RTW_ERR_INVALID = -1,       /* bad argument / handle */
    RTW_ERR_NO_DEVICE = -2,     /* no usable HIP device */
    RTW_ERR_HIP = -3,           /* a HIP runtime call failed */
    RTW_ERR_IO = -4,            /* file could not be read / written */
    RTW_ERR_STATE = -5,         /* scene not committed, etc. */
    RTW_ERR_LIMIT = -6          /* exceeds a compiled-in limit (RTW_MAX_*) */
} rtw_status;

#define RTW_MAX_BOUNCE 16          /* deepest MaxBounceTimes the device path stack holds */
#define RTW_MAX_MATERIAL_NODES 64
#define RTW_MAX_MESH_MATERIALS 64  /* distinct usemtl names per mesh */
#define RTW_UNIT_TABLE_SIZE 0xFFFFFFu   /* MaxUnitVectorNums, Src/Math.cpp:17 */

/* Flattened ISurfaceMaterial tree (Src/SurfaceMaterials.h:47-141); root is node 0 and
 * children always have larger indices than their parent. */
typedef enum {
    RTW_MAT_DIFFUSE = 0,          /* SurfaceMaterial_Diffuse(albedo)                      */
    RTW_MAT_DIFFUSE_CHECKER = 1,  /* SurfaceMaterial_DiffuseChecker(albedo, param=size)   */
    RTW_MAT_REFLECTIVE = 2,       /* SurfaceMaterial_Reflective(albedo, param=fuzziness)  */
    RTW_MAT_EMISSIVE = 3,         /* SurfaceMaterial_Emissive(colour)                     */
    RTW_MAT_BLEND = 4,            /* SurfaceMaterial_Blend(A, B, param=factor)            */
    RTW_MAT_COMBINE = 5,          /* SurfaceMaterial_Combine(A, B)                        */
    RTW_MAT_NULL = 6              /* SurfaceMaterial_Null                                 */
} rtw_material_type;

typedef struct {
    int32_t type;
    float r, g, b;
    float param;
    int32_t child_a, child_b;
    int32_t pad;
} rtw_material_node;              /* 32 bytes */

typedef struct {
    uint64_t rays;          /* FindIntersectionWithScene-equivalent queries            */
    uint64_t box_tests;     /* node / shape box tests actually executed                */
    uint64_t tri_tests;     /* triangle tests executed                                 */
    uint64_t shaded_hits;   /* hits that ran the shading-input block                   */
    uint64_t tex_samples;   /* bilinear texture samples                                */
    uint64_t camera_rays;
} rtw_stats;

typedef struct rtw_context rtw_context;
typedef struct rtw_scene rtw_scene;
typedef struct rtw_framebuffer rtw_framebuffer;

/* ---- context: one per (process, GPU).  Replaces the process-global state of
 * RayTracerProgram::Run (Src/RayTracerProgram.cpp:437-443: srand + the unit-vector table
 * of RMath::InitPseudoRandomUnitVector, Src/Math.cpp:24-31). ---- */
int rtw_context_create(int device_index, rtw_context** out);
int rtw_context_destroy(rtw_context* ctx);
/* run every later launch of this context on the caller's hipStream_t (e.g. torch's) */
int rtw_context_set_stream(rtw_context* ctx, void* hip_stream);
int rtw_context_synchronize(rtw_context* ctx);
/* Switches; results never depend on them (every combination is tested bit-identical).
 *   "pipeline"      4 (default) = pass-batched: the passes of one rtw_render_passes call are rendered in groups that share one set of launches (screen
 *                   bins for the camera rays, a ray per lane for the bounce rounds; rtw_group_kernels.h), every frame shape, pixel range and scene;
 *                   3 = one pass per set of launches: screen bins for the camera rays + one wave-per-ray trace launch and one shade launch per bounce
 *                   (the one-pass reference the pass-batched pipeline is compared with); 0 = one kernel, one thread per pixel (with
 *                   rtw_scene_set_traversal(0): the reference's own visit order, for the work counters).
 *   "group_max" (256) passes per group at most (a power of two), "group_paths" (32 Mi) paths a launch should hold; "group_split" (1) a group of at least
 *                   "split_min" (8) passes runs as up to "group_parts" (2; at most 4) parts of at least "split_paths" (400 000) paths each, on as many streams
 *                   (a workspace per part);
 *   "wave_below" (80 000; x 5 for trees of more than 4 096 nodes) a trace round with fewer rays runs a wave per ray; "visit_budget" (384) one-mesh scenes:
 *                   a ray's node visits in the ray-per-lane kernel before it goes to the wave-per-ray one (a rare ray that walks a thousand nodes kept its
 *                   whole wave waiting), for trees with more than "budget_nodes" (0) nodes;
 *   "backface_filter" (1) one-mesh scenes whose tree fits LDS: the persistent trace blocks also stage the triangles' planes and never note a leaf whose
 *                   triangle faces away from the ray's origin (RRay::TestIntersectionWithTriangle's first rejection, which does not depend on the segment);
 *   "primary_passes" (0 = chosen per launch; 1..4; -1 = one ray set at a time) one-mesh scenes: passes of a tile one wave of the primary kernel takes, its bin
 *                   walked once for up to four rays per lane (sub-samples x passes <= 4); "sky_blocks" (4) blocks of the sky kernel per CU at most;
 *   "workspace_limit_mb" (0 = 24 GiB) a group's workspace may not exceed this: larger groups are re-formed smaller (see rtw_context_memory_bytes);
 *   "device_build" (1) tree, layouts and screen bins built on the device; "hint_period" (16) pipeline 3: the queue lengths that size the next launches
 *                   are read back every n-th pass; "kernel_timing" 1 = record events around the stages of each pass / group (rtw_last_pass_kernel_ms);
 *   "denoise_tiling" (-1) which tiling each level of rtw_denoise runs: 0 = dense, 1 = lattice, -1 = the measured rule; the result is the same bits;
 *   "variance_prefilter" (-1) where rtw_denoise_variance's levels get the prefiltered variance g from: 0 = fetched by the level kernels, 1 = a prefilter launch
 *                   per level, -1 = the measured rule; same bits;
 *   "reproject_staging" (-1) where rtw_reproject's taps come from: 0 = global memory, 1 = the block's tap box staged in LDS, -1 = the measured rule; same bits;
 *   "upsample_staging" (-1) where rtw_upsample's taps come from: 0 = global memory, 1 = the tile's box of low-resolution records staged in LDS, -1 = the measured rule; same bits;
 *   "tonemap_histogram" (-1) how a wave of rtw_tonemap / rtw_exposure_meter builds its histogram in LDS: 0 = an atomic per lane, 1 = one addition per distinct
 *                   bin of the wave's pixels, -1 = the measured rule; same bits;  "tonemap_blocks" (0) > 0: those calls launch at most this many blocks;
 *   "query_kernel"  (-1) which kernel the device queries (rtw_trace_closest_device / rtw_trace_occluded_device / rtw_trace_occluded) run: 1 = the ray-per-lane
 *                   query kernel (rtw_query_kernels.h); 0 = the kernel of rtw_trace_closest on the caller's buffers (any-hit: a closest query whose
 *                   shape >= 0 becomes the byte) -- the A/B baseline and cross-check; -1 = the measured rule (profiles/query_experiments.md): any-hit on
 *                   one-mesh scenes runs the query kernel, everything else the old one.  Results never depend on it, nor on the next;
 *   "query_blocks"  (0 = one grid sized from the device's compute units) > 0: at most exactly that many blocks, so that few rays make many trips of
 *                   the query kernel's batch loop;
 *   "lens_route"    (-1) pipeline 4, scenes with a lens (rtw_scene_set_lens): 1 = the camera round -- glens_kernel makes the lens rays, a lane per path, and
 *                   the ray-per-lane trace kernels of the bounce rounds find their hits in a round of its own ahead of round 0; 0 = gprimary_kernel's LENS
 *                   instantiation, which walks the trees itself a tile per wave; -1 = the measured rule (profiles/lens_experiments.md): route 0, which
 *                   won on every scene measured -- the camera round is kept as the cross-check.  Results never depend on it;
 *   "material_variants" (1) pipeline 4: the shade and primary kernels are instantiated for the scene's material class (RTW_MATERIAL_CLASS_*, worked out by
 *                   rtw_scene_commit); 0 = the general instantiation for every scene, the A/B baseline and cross-check.  Results never depend on it. */
int rtw_context_set_option(rtw_context* ctx, const char* name, int value);
/* with option "kernel_timing" = 1: HIP-event durations (ms) of the latest pass's three stages -- primary kernel(s),
 * the per-bounce trace / shade launches, resolve -- measured on the context's stream; waits for that pass. */
int rtw_last_pass_kernel_ms(rtw_context* ctx, float out3[3]);
/* passes the latest group of the pass-batched pipeline held (rtw_last_pass_kernel_ms times that group) */
int rtw_last_group_passes(rtw_context* ctx);
/* the pipeline the latest render call of this context actually ran (0, 3 or 4; -1 before the first call): lets a caller see a fallback */
int rtw_last_pass_pipeline(rtw_context* ctx);
/* Material classes.  FLAT: every shape of the scene has a material tree of exactly one node, a Diffuse or a DiffuseChecker, and no mesh has a valid
 * texture; FLAT_TEX: the same trees, some mesh textured; GENERAL: every other scene -- and every call with work counters on (rtw_stats_enable), with a
 * sphere / plane / capsule / triangle in the scene or with a lens, for which no specialised kernels are built. */
#define RTW_MATERIAL_CLASS_GENERAL 0
#define RTW_MATERIAL_CLASS_FLAT 1
#define RTW_MATERIAL_CLASS_FLAT_TEX 2
/* the material class the shade / primary kernels of the latest pipeline-4 call of this context were instantiated for (-1 before the first such call):
 * lets a caller see that a flat scene did get its kernels, and that option "material_variants" 0 did switch them off */
int rtw_last_pass_material_class(rtw_context* ctx);
const char* rtw_last_error(void);
const char* rtw_version(void);

/* ---- scene: RayTracerScene (Src/RayTracerScene.h:43-62) ---- */
int rtw_scene_create(rtw_context* ctx, rtw_scene** out);
int rtw_scene_destroy(rtw_scene* scene);
/* RayTracerScene::AddShape(RMeshShape::Create(path), ...) : OBJ + sibling MTL + PNG
 * textures with the reference's parser semantics (Src/MeshShape.cpp:65-278). */
int rtw_scene_add_mesh_obj(rtw_scene* scene, const char* obj_path, int* out_shape);
/* RayTracerScene::AddShape(RSphere::Create(center, radius), ...) / RPlane::Create(normal, point) / RCapsule::Create(start, end,
 * radius) (Src/Shapes.h:46-112; intersections Src/RRay.cpp:25-87 and Src/Shapes.cpp:18-125).  Shapes keep their insertion order
 * (it decides which of two hits at one distance wins, and which hit's sampled colour a later sphere / plane / capsule-side hit
 * inherits: one RayHitResult serves all shapes of a query, Src/RayTracerScene.cpp:99-125).  A plane has no culling box
 * (RPlane::HasCullingBounds).  The material is set with rtw_scene_set_material as for a mesh. */
int rtw_scene_add_sphere(rtw_scene* scene, const float center[3], float radius, int* out_shape);
int rtw_scene_add_plane(rtw_scene* scene, const float normal[3], const float point[3], int* out_shape);
int rtw_scene_add_capsule(rtw_scene* scene, const float start[3], const float end[3], float radius, int* out_shape);
/* RTriangle::Create(p0, p1, p2) (Src/Shapes.h:106-130): one single-sided triangle with its face normal, culled by the box of its
 * three points (so an axis-aligned one is as invisible as the reference's: its zero-thickness box never passes the slab test). */
int rtw_scene_add_triangle(rtw_scene* scene, const float p0[3], const float p1[3], const float p2[3], int* out_shape);
/* Same, from arrays the caller already holds (the members of RMeshShape,
 * Src/MeshShape.h:25-37).  positions/texcoords/normals are 3 floats per element,
 * idx_* are 3 ints per triangle (0-based), tri_material is 1 int per triangle (-1 = none).
 * shape_bounds6 may be NULL (then the bounds of all positions, Src/MeshShape.cpp:109). */
int rtw_scene_add_mesh(rtw_scene* scene,
                       const float* positions, int n_positions,
                       const float* texcoords, int n_texcoords,
                       const float* normals, int n_normals,
                       const int32_t* idx_p, const int32_t* idx_t, const int32_t* idx_n,
                       const int32_t* tri_material, int n_tris,
                       const float* shape_bounds6, int* out_shape);
/* RTexture::LoadTexturePNG result for one material id (Src/Texture.cpp:119-151):
 * 8-bit texels, channels 3 (RGB, alpha = 1) or 4 (RGBA), row-major, top row first. */
int rtw_scene_set_texture(rtw_scene* scene, int shape, int material_id,
                          const uint8_t* texels, int width, int height, int channels);
/* RShape::SetSurfaceMaterial (Src/Shapes.cpp:9) */
int rtw_scene_set_material(rtw_scene* scene, int shape, const rtw_material_node* nodes, int n_nodes);
/* build + flatten + upload; the scene is immutable afterwards (all reference queries are const) */
int rtw_scene_commit(rtw_scene* scene);
/* info[0..7] = points, texcoords, normals, triangles, materials, nodes, textures, max tree depth */
int rtw_scene_mesh_info(const rtw_scene* scene, int shape, int32_t info[8], float shape_bounds6[6]);
/* flattened tree for inspection: per node 6 floats (min, max), skip index, triangle (-1 internal) */
int rtw_scene_mesh_nodes(const rtw_scene* scene, int shape, float* bounds6, int32_t* skip, int32_t* tri, int max_nodes);
/* traversal pruning (result-preserving segment clip); default on */
int rtw_scene_set_prune(rtw_scene* scene, int enabled);
/* 1 (default): screen bins, link tree and flat hierarchy may be used (candidate leaves gathered in the reference's order before their
 * triangle tests); 0: every ray walks the binary tree in preorder, visiting exactly the boxes KdNode::TestRayIntersection
 * visits (Src/KdTree.cpp:128-195; one thread per pixel; used for reference-faithful work counters).  Same results. */
int rtw_scene_set_traversal(rtw_scene* scene, int mode);
/* The flat hierarchy over the leaves in preorder that the wave-per-ray walk uses: level 0 = each
 * leaf's own box (KdNode::Bounds of the leaf, Src/KdTree.cpp:37-60), level 1 / 2 = unions of 16 /
 * 256 consecutive leaves.  boxes6 = min.xyz, max.xyz per entry.  Returns the level's entry count. */
int rtw_scene_mesh_flat(const rtw_scene* scene, int shape, int level, float* boxes6, int max_entries);
/* ---- camera ----
 * Pixel (x, y) of a width x height frame, sub-sample offset (ox, oy) (Src/RayTracerProgram.cpp:141-162: dx, dy, the quarter-pixel
 * offsets and the two jitter draws) looks from `eye` along
 *     v[k] = (right[k] * (dx + ox) + up[k] * (dy + oy)) + forward[k] * focal        (k = 0, 1, 2; every product and sum rounded on its own)
 *     dir  = v * (1.0f / sqrtf(v.x * v.x + v.y * v.y + v.z * v.z)),   distance 1000.
 * The reference's one camera is the default: eye (0, 0, 7), right (1, 0, 0), up (0, 1, 0), forward (0, 0, -1), focal 0.5; a scene
 * whose camera equals it bit for bit renders through the fixed-pose kernels (the images, and the code, of a scene that never set one).
 * The kernels use the struct's floats as given: the handedness of the basis is not checked, and a left-handed one (right = -cross(forward, up))
 * renders the mirrored image without an error.  rtw_camera_look_at always returns a right-handed basis. */
typedef struct { float eye[3], right[3], up[3], forward[3]; float focal; } rtw_camera;
int rtw_camera_default(rtw_camera* out);
/* forward = normalized(target - eye), right = normalized(cross(forward, up_hint)), up = cross(right, forward),
 * focal = 0.25 / tan(vfov / 2) (the reference's 0.5 is vfov = 2 atan(0.5) ~ 53.13 degrees).  RTW_ERR_INVALID for a non-finite
 * argument, vfov outside (0, 180), target == eye, or an up_hint parallel to forward. */
int rtw_camera_look_at(const float eye[3], const float target[3], const float up_hint[3], float vfov_degrees, rtw_camera* out);
/* The camera every render call of this scene uses from now on (NULL = the default).  Before or after commit, and between render
 * calls: after commit it waits for the context's streams and drops the scene's cached screen bins and tile tables (they are rebuilt
 * for the new pose on the next render call).  RTW_ERR_INVALID for non-finite values, focal <= 0, or a basis whose vectors are
 * not unit length and mutually orthogonal to within 1e-4. */
int rtw_scene_set_camera(rtw_scene* scene, const rtw_camera* cam);
int rtw_scene_get_camera(const rtw_scene* scene, rtw_camera* out);
/* The camera rays of n pixels (pixel = y * width + x) as the render kernels build them, jitter included: 7 floats each (origin,
 * direction, distance), the layout rtw_trace_closest / rtw_ray_trace take.  Host only, needs no context. */
int rtw_camera_rays(const rtw_camera* cam, int width, int height, const int32_t* pixels, int64_t n,
                    int pass_index, int sub_sample, uint32_t seed, float* rays7);

/* ---- thin lens: depth of field ----
 * A lens of radius aperture_radius (world units) at the eye, in the plane of `right` and `up`, focused on the plane focus_distance along `forward`:
 * a point of that plane is sharp, everything else is blurred by its circle of confusion.  aperture_radius == 0 is the pinhole exactly: the same
 * kernel instantiations, the same screen bins, the same images bit for bit.  For aperture_radius > 0 a sample's ray is (float32, every product and
 * every sum rounded on its own):
 *   1. a = dx + ox, b = dy + oy and v[k] as for the camera above, jitter draws (counters 0 and 1 of the path's stream) included; the path's counter
 *      stands at 2 afterwards, with or without a lens, so no later random decision of any path changes.
 *   2. the lens point from a stream of its own, key_l = stream_key(seed, pixel, (pass_index * 4 + sub_sample) | 0x80000000u): for try t = 0 .. 7
 *      lx = 2 u(2t) - 1, ly = 2 u(2t + 1) - 1 with u(c) = (float)(int32)(mix32(key_l + c) >> 1) / 2147483648.0f; the first try with
 *      lx * lx + ly * ly <= 1.0f is taken; if none of the eight is (4.5e-6 of the samples), lx = ly = 0.
 *      pass_index must stay below 2^29 with a lens (RTW_ERR_LIMIT above): bit 31 of the sample word belongs to the lens stream.
 *   3. s = focus_distance / focal;  lxr = lx * aperture_radius, lyr = ly * aperture_radius;  off[k] = right[k] * lxr + up[k] * lyr;
 *      origin[k] = eye[k] + off[k];  w[k] = v[k] * s - off[k];  dir = w * (1.0f / sqrtf((w.x * w.x + w.y * w.y) + w.z * w.z)),  distance 1000.
 * With a lens no mesh gets screen bins (the projection from `eye` no longer bounds what a tile's rays can meet: rtw_scene_mesh_bins returns 0),
 * every tile is rendered as a busy one, and the workspace of the pass-batched pipeline is sized for all pixels of the frame. */
typedef struct { float aperture_radius; float focus_distance; } rtw_lens;   /* world units; focus_distance measured along `forward` */
/* The lens every render call of this scene uses from now on (NULL or aperture_radius == 0: the pinhole).  Before or after commit and between render
 * calls, like rtw_scene_set_camera: after commit it waits for the context's streams and drops the scene's cached screen bins and tile tables.
 * RTW_ERR_INVALID for a non-finite value, aperture_radius < 0 or focus_distance <= 0. */
int rtw_scene_set_lens(rtw_scene* scene, const rtw_lens* lens);
int rtw_scene_get_lens(const rtw_scene* scene, rtw_lens* out);
/* rtw_camera_rays through a lens (NULL or aperture_radius == 0: rtw_camera_rays bit for bit).  Host only, needs no context. */
int rtw_lens_rays(const rtw_camera* cam, const rtw_lens* lens, int width, int height, const int32_t* pixels, int64_t n,
                  int pass_index, int sub_sample, uint32_t seed, float* rays7);

/* Screen-space bins of the scene's current camera (the reference's: Src/RayTracerProgram.cpp:133-165) for a
 * width x height frame cut into bin_w x bin_h pixel bins: CSR offsets (bins + 1) and, per bin, the
 * node indices (ascending) of the leaves whose triangle a camera ray of the bin's pixels could accept
 * (it faces the camera by the reference's own float test and its projection touches the bin).
 * counts2 = {number of offsets, number of entries}.  Returns 1, or 0 when this mesh gets no bins. */
int rtw_scene_mesh_bins(const rtw_scene* scene, int shape, int width, int height, int bin_w, int bin_h,
                        uint32_t* offsets, int64_t max_offsets, uint32_t* entries, int64_t max_entries, int64_t* counts2);

/* ---- ray-level queries (parity surface) ---- */
/* RayTracerScene::FindIntersectionWithScene (Src/RayTracerScene.cpp:99-125) for n rays.
 * rays: 7 floats each (origin, direction, distance).  hits: 11 floats each (HitPosition,
 * HitNormal, Distance, SampledColor, SampledAlpha); shape/tri: hit shape index (-1 miss)
 * and original triangle index.  Host buffers. */
int rtw_trace_closest(rtw_scene* scene, const float* rays, int64_t n,
                      float* hits11, int32_t* shape, int32_t* tri);
/* ---- ray queries on device buffers: closest-hit and any-hit, asynchronous on the context's stream ---- */
/* FindIntersectionWithScene for n rays that already live in device memory.  rays_dev: n x 7 floats (origin, direction, distance),
 * hits11_dev: n x 11 floats, shape_dev / tri_dev: n int32 -- the layouts of rtw_trace_closest, byte for byte the values it returns
 * (misses included).  Any output may be NULL (not stored); at least one must not be.  Asynchronous on the context's stream:
 * no allocation, no copy, no synchronisation.  The pointers are the caller's (as for rtw_framebuffer_wrap): 4-byte aligned, dense,
 * inputs and outputs not overlapping.  At most 2^31 - 1 rays per call (RTW_ERR_LIMIT above).
 * Where the old kernel runs ("query_kernel" 0, or -1 and the rule picks it) and an output is NULL -- or for any-hit -- the old kernel's outputs
 * go to a stand-in buffer of the context: the first such call, and one with more rays than any before, waits for the stream and allocates. */
int rtw_trace_closest_device(rtw_scene* scene, const void* rays_dev, int64_t n, void* hits11_dev, void* shape_dev, void* tri_dev);
/* occluded_dev: n bytes, 1 when rtw_trace_closest would report shape >= 0 for the ray, else 0.  The geometric test only: a texel's alpha
 * plays no part (it does not in FindIntersectionWithScene either).  A lane stops at its first accepted hit. */
int rtw_trace_occluded_device(rtw_scene* scene, const void* rays_dev, int64_t n, void* occluded_dev);
/* the same from / to host arrays (stages through device memory and waits, like rtw_trace_closest) */
int rtw_trace_occluded(rtw_scene* scene, const float* rays, int64_t n, uint8_t* occluded);
/* DIAGNOSTIC (tests size a batch larger than one grid sweep with it): threads per block (out2[0]) and blocks (out2[1]) the device queries above launch for n rays with the context's current options
 * (any_hit: 0 = closest, 1 = occluded); where the old kernel runs: 256 and ceil(n / 256) */
int rtw_query_launch_shape(rtw_scene* scene, int64_t n, int any_hit, int32_t out2[2]);
/* RayTracerScene::RayTrace (Src/RayTracerScene.cpp:31-97) for n explicit rays; keys2 holds
 * (pixel, sample) per ray, which select the random stream.  rgb: 3 floats each. */
int rtw_ray_trace(rtw_scene* scene, const float* rays, const uint32_t* keys2, int64_t n,
                  int max_bounce, int use_base_color, uint32_t seed, int width, int height, float* rgb);
/* RTexture::Sample (Src/Texture.cpp:23-57) probes: uv 2 floats each -> rgba 4 floats each */
int rtw_texture_sample(rtw_scene* scene, int shape, int material_id, const float* uv, int64_t n, float* rgba);

/* ---- framebuffer: accuBuffer[] + bitcolor[] (Src/RayTracerProgram.cpp:49-77) ---- */
int rtw_framebuffer_create(rtw_context* ctx, int width, int height, rtw_framebuffer** out);
/* wrap caller-owned device memory: accum = width*height*16 bytes (sum.xyz, int count),
 * argb = width*height*4 bytes.  Lets torch own the buffers that RCCL gathers. */
int rtw_framebuffer_wrap(rtw_context* ctx, int width, int height, void* accum_dev, void* argb_dev, rtw_framebuffer** out);
int rtw_framebuffer_destroy(rtw_framebuffer* fb);
int rtw_framebuffer_clear(rtw_framebuffer* fb);
/* copy out: accum4 = width*height*4 floats (sum.xyz, count as float); argb = 0xAARRGGBB */
int rtw_framebuffer_read_float(rtw_framebuffer* fb, float* accum4);
int rtw_framebuffer_resolve_argb(rtw_framebuffer* fb, uint32_t* argb);
/* the device addresses of the two arrays (accum: width*height float4 = sum.xyz + int count; argb: width*height 0xAARRGGBB words), e.g. for a display
 * hook that blits bitcolor[] straight out of device memory (Src/Windows/RenderWindow.cpp:150-187 blits the host array); valid while the framebuffer
 * lives; order reads after the renders on the context's stream.  Either pointer argument may be NULL. */
int rtw_framebuffer_device_pointers(rtw_framebuffer* fb, void** accum_dev, void** argb_dev);

/* ---- the hot path ---- */
/* ThreadWorker_Render(begin, end, MaxBounceCount, RenderOption{use_base_color})
 * (Src/RayTracerProgram.cpp:131-188) for one pass: pixel indices begin..end INCLUSIVE,
 * row-major.  sub_samples in 1..4 (the reference always uses 4); pass_index and seed
 * select the random streams.  Asynchronous on the context's stream; calls on disjoint
 * ranges may be issued back to back. */
int rtw_render_range(rtw_scene* scene, rtw_framebuffer* fb, int begin, int end, int max_bounce,
                     int use_base_color, int pass_index, int sub_samples, uint32_t seed);
/* One pass over this rank's share of the frame: the reference's NumTaskRows-row tasks
 * (Src/RayTracerProgram.cpp:282,294-301) dealt round-robin, task t belongs to rank
 * t % world.  Pixels keep their global indices (and random streams), so the image is
 * identical for every world size. */
int rtw_render_tasks(rtw_scene* scene, rtw_framebuffer* fb, int task_rows, int rank, int world,
                     int max_bounce, int use_base_color, int pass_index, int sub_samples, uint32_t seed);
/* UpdateBitmapPixels' sample loop (Src/RayTracerProgram.cpp:317-361): n_passes accumulated passes
 * first_pass .. first_pass + n_passes - 1 over this rank's tasks, as rtw_render_tasks would render
 * them one by one (same final images).  The passes are rendered in groups that share one set of launches; a pixel's pass colours are
 * added to its accumulator one by one in pass order, its accumulator entry is written and its ARGB word (divide + gamma of the accumulator after
 * the group's last pass) computed and written once per group: intermediate images are not materialised inside a call (call it with
 * n_passes = 1 to show every pass). */
int rtw_render_passes(rtw_scene* scene, rtw_framebuffer* fb, int task_rows, int rank, int world,
                      int max_bounce, int use_base_color, int first_pass, int n_passes,
                      int sub_samples, uint32_t seed);
/* Per-pixel pass budgets (adaptive sampling; no reference counterpart): rtw_render_passes with a pass count of each pixel's own.  budget_dev: width x
 * height int32 in device memory, index py * width + px, read asynchronously on the context's streams (the caller orders its writes on the context's
 * stream, as for rtw_trace_*_device).  With e(p) = min(max(budget[p], 0), n_passes), pixel p of this rank's tasks receives the passes
 * first_pass .. first_pass + e(p) - 1 and nothing else: afterwards its accumulator entry and its ARGB word are, bit for bit, what
 * rtw_render_passes(.., use_base_color = 0, first_pass, e(p), ..) leaves in that pixel from the same starting framebuffer (a pixel's pass is keyed by
 * seed, pixel, pass and sub-sample alone, and every pixel carries its own pass count).  A pixel with e(p) == 0, or of another rank, is not written.
 * Pipeline 4 only; groups, split groups, workspace and the fallback to smaller groups are those of rtw_render_passes with the same n_passes
 * (rtw_render_reserve with the same arguments covers the call); paths that are not started leave their workspace slots unused, nothing is compacted and
 * the host never waits to learn a count.  With a lens the camera rays take route 0 whatever "lens_route" says.  There is no preview mode.
 * rtw_last_pass_pipeline, rtw_last_group_passes and rtw_last_pass_material_class report as for rtw_render_passes.
 * RTW_ERR_INVALID, nothing launched: budget_dev null, a bad pass range, option "pipeline" 3 or 0 (or a scene on traversal 0), work counters enabled
 * (rtw_stats_enable); every other error is rtw_render_passes', the 2^29 limit under a lens included. */
int rtw_render_passes_budget(rtw_scene* scene, rtw_framebuffer* fb, const void* budget_dev, int task_rows, int rank, int world,
                             int max_bounce, int first_pass, int n_passes, int sub_samples, uint32_t seed);

/* Prepare, without rendering, everything a later rtw_render_passes call with these arguments would otherwise make inside it: the screen bins and tile
 * tables of this frame shape and the workspace of the largest group of passes that call will form (the workspace is grow-only; growing it waits for the
 * context's streams -- measured 0.3 ms inside a timed call).  UpdateBitmapPixels has no counterpart: its buffers are static arrays. */
int rtw_render_reserve(rtw_scene* scene, rtw_framebuffer* fb, int task_rows, int rank, int world,
                       int max_bounce, int n_passes, int sub_samples);
/* ---- first-hit feature buffers: depth, normal, albedo and ids per pixel (what a denoiser, a compositor or a picking tool asks for first) ----
 * No reference counterpart (the nearest thing is its UseBaseColor preview pass).  Take pixel p, pass k and sub-sample i: the SAMPLE RAY is exactly the
 * camera ray the render kernels build for (p, k, i, seed) under the scene's current camera and lens -- rtw_lens_rays' ray bit for bit.
 * FindIntersectionWithScene of that ray gives the sample's values:
 *     depth            Result.Distance (along the ray from its origin, not a z-depth);                    a miss: the ray's own distance, 1000.0f
 *     normal           Result.HitNormal (the world-space shading normal rtw_trace_closest reports);       a miss: (0, 0, 0)
 *     albedo           RayTrace(ray, 1, RenderOption{UseBaseColor = true}) = PreviewColor(Result) * Result.SampledColor, the shared-RayHitResult colour
 *                      inheritance included; a texel's alpha plays no part;                               a miss: the sky colour
 *     shape, triangle  what rtw_trace_closest reports for the ray;                                        a miss: -1, -1
 * Per pass and pixel each of the seven float channels takes c = (v_0 + v_1 + ... + v_{ns-1}) / ns -- summed left to right in float32 from +0, no division
 * when ns == 1 (the shape of ThreadWorker_Render's pass colour); per call, for the passes in order: sum += c, count += 1 (AccumulatePixel::AddPixel).
 * The ids are those of sub-sample 0 of the LAST pass of the call.  Three buffers, 40 bytes per pixel:
 *     geom    float4   (sum normal.xyz, sum depth)
 *     albedo  float4   (sum albedo.rgb, int count in the bits of w, like the accumulator)
 *     ids     int32 x 2 (shape, triangle)
 * A call touches only the pixels of this rank's tasks (dealt as rtw_render_passes deals them); calls accumulate until rtw_features_clear.  The result
 * depends on the scene, camera, lens, frame shape, sub_samples, passes and seed only -- never on an option of the context or the scene. */
typedef struct rtw_features rtw_features;
int rtw_features_create(rtw_context* ctx, int width, int height, rtw_features** out);
/* wrap caller-owned device memory (e.g. torch tensors): geom and albedo width*height*16 bytes, 16-byte aligned; ids width*height*8 bytes, 8-byte aligned */
int rtw_features_wrap(rtw_context* ctx, int width, int height, void* geom_dev, void* albedo_dev, void* ids_dev, rtw_features** out);
int rtw_features_destroy(rtw_features* f);
/* all sums and counts to zero, ids to (-1, -1); asynchronous on the context's stream */
int rtw_features_clear(rtw_features* f);
/* copy out (any pointer may be NULL): geom4 / albedo4 = width*height*4 floats, the count returned as a float like rtw_framebuffer_read_float; ids2 = width*height*2 */
int rtw_features_read(rtw_features* f, float* geom4, float* albedo4, int32_t* ids2);
int rtw_features_device_pointers(rtw_features* f, void** geom_dev, void** albedo_dev, void** ids_dev);
/* Passes first_pass .. first_pass + n_passes - 1 of this rank's tasks into f.  Asynchronous on the context's stream: one or two launches, and no allocation,
 * copy or synchronisation once the frame shape's screen bins and tile tables exist (the cached tables of rtw_render_passes, built the same way when they are
 * missing).  RTW_ERR_STATE for an uncommitted scene; RTW_ERR_INVALID for bad sizes, counts or handles or a features object of another context;
 * RTW_ERR_LIMIT for a pass index >= 2^29 with a lens.  rtw_scene_set_camera / rtw_scene_set_lens between calls behave as for rendering.  The work
 * counters (rtw_stats) are not touched. */
int rtw_render_features(rtw_scene* scene, rtw_features* f, int task_rows, int rank, int world,
                        int first_pass, int n_passes, int sub_samples, uint32_t seed);

/* ---- edge-avoiding a-trous denoiser over a framebuffer and its feature buffers (Dammertz et al. 2010; no reference counterpart) ----
 * An image-space filter guided by the first-hit features, with the base colour divided out first so that textures stay sharp.  It takes buffers and no
 * scene, so it serves any image the caller can describe this way.  src: accum = (sum.xyz, int count_fb); f: geom = (sum normal.xyz, sum depth), albedo =
 * (sum rgb, int count_f), ids = (shape, triangle); dst: another framebuffer.  Same width and height, same context, dst != src.  Per pixel
 *     C = accum.xyz / count_fb      n = geom.xyz / count_f (not renormalised)      z = geom.w / count_f      A = albedo.rgb / count_f      s = shape id
 * A pixel is EMPTY when either count is 0 and BAD when a channel of C is not finite.  EPS = 1e-3f.
 * I_0 = C / (A + EPS) per channel with RTW_DENOISE_DEMODULATE, else I_0 = C.  For level i = 0 .. levels-1, step = 2^i, for every non-empty pixel p:
 *     sw = 0, sc = 0
 *     for dy = -2..2, for dx = -2..2            (in this order)
 *         q = p + step * (dx, dy)
 *         skip q when it is outside the frame, empty or bad
 *         skip q when RTW_DENOISE_SAME_SHAPE is set and s_q != s_p
 *         e = 0
 *         if sigma_color  > 0 and p is not bad:  e += |I_i(p) - I_i(q)|^2 / (sigma_color * 2^-i)^2
 *         if sigma_normal > 0:                   e += |n_p - n_q|^2 / sigma_normal^2
 *         if sigma_depth  > 0:                   e += ((z_p - z_q) / (sigma_depth * max(|z_p|, 1e-6)))^2
 *         w = h[dx] * h[dy] * exp(-e)            h = (1/16, 1/4, 3/8, 1/4, 1/16)
 *         sw += w;  sc += w * I_i(q)
 *     I_{i+1}(p) = sc / sw   when sw > 0
 *                  I_i(p)    when sw == 0 and p is not bad
 *                  0         otherwise
 * out = I_levels * (A + EPS) with RTW_DENOISE_DEMODULATE, else I_levels; an empty pixel gives (0, 0, 0).  dst.accum takes (out.xyz, count 1), dst.argb
 * the gamma pack of out (the thresholds of rtw_gamma_thresholds): dst is then an ordinary one-pass framebuffer for every other call.  src and f are not
 * written.  A non-positive sigma switches its term off.  Misses (depth 1000, normal 0, id -1) are their own "surface".  Everything is float32, the taps
 * are summed in the stated order, exp(-e) is the hardware exp2 of -e * log2(e); shape ids are compared in their low 30 bits.
 * Asynchronous on the context's stream: 1 + levels launches.  The work space (two float4 images and a 20-byte guide record per pixel, 52 bytes per
 * pixel) belongs to the context, grows only, is counted by rtw_context_memory_bytes and released by rtw_context_trim: a repeated call of the same size
 * does no allocation, copy or synchronisation.  The context option "denoise_tiling" (-1) picks each level's tiling -- 0 = dense tiles with a halo,
 * 1 = tiles of the step's lattices, -1 = the faster by measurement -- and never changes a result: both give the same bits.
 * RTW_ERR_INVALID: a null handle, differing sizes, handles of different contexts, dst == src, levels outside 1..6, a NaN sigma, unknown flag bits. */
#define RTW_DENOISE_DEMODULATE 1u
#define RTW_DENOISE_SAME_SHAPE 2u
typedef struct rtw_denoise_params { int levels; float sigma_color, sigma_normal, sigma_depth; uint32_t flags; } rtw_denoise_params;
/* 5 levels, both flags, sigma_color 0.6 (on the demodulated colour, i.e. in units of the surface's own brightness; halved per level as the paper does),
 * sigma_normal 0.3 (|n_p - n_q| of about 17 degrees costs a factor e), sigma_depth 0.1 (a relative distance step of 10 % costs a factor e) */
int rtw_denoise_default_params(rtw_denoise_params* p);
int rtw_denoise(rtw_framebuffer* src, rtw_features* f, const rtw_denoise_params* p, rtw_framebuffer* dst);

/* ---- temporal reprojection: accumulate frames across camera moves (the temporal half of SVGF, Schied et al. 2017; no reference counterpart) ----
 * Each pixel's first hit is projected into the previous camera, the history is fetched there, kept only where it shows the same surface, and blended
 * with the new sample.  It takes buffers and cameras and no scene.  cur / f_cur: the current frame (one or more passes) and its features under cam_cur;
 * hist / f_hist: the accumulated history and the features of the frame it was made from, under cam_prev; dst: another framebuffer.  The caller keeps two
 * framebuffers and two feature objects and swaps them each frame: dst is the next frame's hist, f_cur the next f_hist.  A cleared hist means "no history".
 * dst is an ordinary framebuffer whose count is the history length N: rtw_denoise(dst, f_cur, ...), read, resolve and save all work on it.
 * Everything is float32 unless stated, every product and sum rounded on its own.  For pixel p = (x, y) of the current frame C, n, z, A, s are as in
 * rtw_denoise (sums divided by their counts, shape id in its low 30 bits, EPS = 1e-3f); likewise C_q ... s_q of pixel q of the history.  p is EMPTY when
 * either current count is 0 and BAD when a channel of C is not finite.  EMPTY gives dst.accum = (0, 0, 0, count 0).  W, H = the frame, aspect = (float)W / (float)H.
 *  1 world point     a = pixel_dx(x, W, aspect) = -(float)(x - W / 2) / (W * 2) * aspect,  b = pixel_dy(y, H) = -(float)(y - H / 2) / (H * 2)   (no sub-sample offset)
 *                    v = (right_cur * a + up_cur * b) + forward_cur * focal_cur,  dir = v * (1 / sqrtf(v.v)),  P = eye_cur + dir * z
 *                    Under a lens this is the pinhole's point: the lens blur makes the history approximate, not wrong.
 *  2 previous frame  d = P - eye_prev,  t = d.forward_prev,  z_exp = sqrtf(d.d);  t <= 0: no history.  Otherwise
 *                    u = (d.right_prev) * focal_prev / t,  w = (d.up_prev) * focal_prev / t
 *                    fx = (float)(W / 2) - u * (2 W) / aspect,  fy = (float)(H / 2) - w * (2 H)      (the inverses of pixel_dx / pixel_dy, integer W / 2)
 *                    a coordinate within 1/64 of an integer is snapped to it: r = rintf(fx); if (fabsf(fx - r) <= 1/64) fx = r -- an unmoved camera then
 *                    reads exactly one tap, and the result does not hinge on which side of an integer rounding fell.  (a.b = (a.x b.x + a.y b.y) + a.z b.z)
 *  3 bilinear taps   x0 = floorf(fx), tx = fx - x0, the same for y; the taps (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1) in this order with the weights
 *                    (1-tx)(1-ty), tx(1-ty), (1-tx)ty, tx ty.  A tap of weight 0 is skipped.
 *  4 validity        a tap q is VALID when it lies in the frame, both history counts are non-zero, C_q is finite, s_q == s_p,
 *                    depth_tolerance <= 0 or |z_q - z_exp| <= depth_tolerance * z_exp,  and  s_p is a miss or normal_cos <= -1 or n_p.n_q >= normal_cos.
 *                    Misses are their own surface, as in the denoiser.
 *  5 history         I_q = C_q / (A_q + EPS) with RTW_REPROJECT_DEMODULATE, else C_q; I_cur likewise.  Over the valid taps in order: sw = sum w,
 *                    Ih = (sum w I_q) / sw, Nh = the smallest history count (hist.accum's) among them.
 *  6 blend           history (sw > 0), p not BAD:  N = min(Nh + 1, max_history),  I = Ih + (I_cur - Ih) / (float)N
 *                    history, p BAD:               I = Ih, N = Nh
 *                    no history, p not BAD:        I = I_cur, N = 1
 *                    no history, p BAD:            (0, 0, 0), count 0
 *                    out = I * (A_cur + EPS) with RTW_REPROJECT_DEMODULATE, else I;  dst.accum = (out * (float)N, int N)
 *                    dst.argb = the gamma pack of accum.xyz / N, the value a resolve of dst gives; a pixel of count 0 packs as black.
 * cur, hist and both feature objects are not written.  Asynchronous on the context's stream: ONE launch, no allocation, copy or synchronisation, no work
 * space.  The context option "reproject_staging" (-1) picks where the taps are read from -- 0 = global memory, 1 = the block's box of taps staged in
 * LDS, -1 = the faster by measurement -- and never changes a bit.  A NULL camera is the default camera.
 * RTW_ERR_INVALID, with the destination untouched: a null handle or params, differing sizes, handles of different contexts, dst == cur, dst == hist,
 * f_cur == f_hist, a camera rtw_scene_set_camera would refuse, a NaN parameter, max_history outside 1..65535, unknown flag bits. */
#define RTW_REPROJECT_DEMODULATE 1u
typedef struct rtw_reproject_params { float depth_tolerance, normal_cos; int max_history; uint32_t flags; } rtw_reproject_params;
/* depth_tolerance 0.05 (the history's distance within 5 % of the expected one), normal_cos 0.9 (normals within about 26 degrees), max_history 32
 * (from there on an exponential average of weight 1/32), RTW_REPROJECT_DEMODULATE */
int rtw_reproject_default_params(rtw_reproject_params* p);
int rtw_reproject(const rtw_camera* cam_cur, const rtw_camera* cam_prev, rtw_framebuffer* cur, rtw_features* f_cur,
                  rtw_framebuffer* hist, rtw_features* f_hist, const rtw_reproject_params* p, rtw_framebuffer* dst);

/* ---- luminance moments and the variance-guided filter: with rtw_reproject, the whole of SVGF (Schied et al. 2017; no reference counterpart) ----
 * rtw_denoise weighs colour differences by one fixed sigma_color.  After rtw_reproject a frame is uneven -- pixels with 32 frames of history beside a
 * disocclusion band of one noisy sample -- and the filter needs to know, per pixel, how noisy the pixel still is.  That estimate is the variance of the
 * luminance, from moments accumulated through the reprojection, or from the neighbourhood where the history is short.
 * lum(v) = (0.2126f * v.x + 0.7152f * v.y) + 0.0722f * v.z.
 *
 * rtw_moments: width * height float2 (mu1, mu2), the running means of the luminance and of its square.  It carries no count: the history length is the
 * framebuffer's count, and the caller swaps the two together.  create / wrap (caller-owned device memory, width*height*8 bytes, 8-byte aligned) /
 * destroy / clear (zeros, asynchronous on the context's stream) / read (mu2 = width*height*2 floats) / device_pointer, as rtw_features. */
typedef struct rtw_moments rtw_moments;
int rtw_moments_create(rtw_context* ctx, int width, int height, rtw_moments** out);
int rtw_moments_wrap(rtw_context* ctx, int width, int height, void* mu_dev, rtw_moments** out);
int rtw_moments_destroy(rtw_moments* m);
int rtw_moments_clear(rtw_moments* m);
int rtw_moments_read(rtw_moments* m, float* mu2);
int rtw_moments_device_pointer(rtw_moments* m, void** mu_dev);
/* rtw_reproject with moments, still ONE launch.  dst receives exactly what rtw_reproject writes for the same arguments -- the same bits in accum and
 * argb, under both settings of "reproject_staging".  For m_dst: l = lum(I_cur) of step 5 (demodulated when the flag is set).  The two-channel image
 * (l, l * l) is blended by steps 1 to 6 without demodulation, with m_hist as its history image, hist.accum's counts as its history lengths and
 * moments_history (1..65535; 5 through the wrappers: a floor of 0.2 on the blend weight, as in the paper) in max_history's place.  A tap's validity
 * is the colour's, so with mu_h = (sum w mu_q) / sw over the colour's valid taps:
 *     history (sw > 0), p not BAD:   mu = mu_h + ((l, l * l) - mu_h) / (float)min(Nh + 1, moments_history)
 *     history, p BAD:                mu = mu_h
 *     no history, p not BAD:         mu = (l, l * l)
 *     no history and p BAD, or p EMPTY:   mu = (0, 0)
 * The projection, the taps and their tests are computed once for both.  m_hist is not written.
 * RTW_ERR_INVALID, with both destinations untouched: whatever rtw_reproject refuses, null moments, moments of another size or context,
 * m_dst == m_hist, moments_history outside 1..65535. */
int rtw_reproject_moments(const rtw_camera* cam_cur, const rtw_camera* cam_prev, rtw_framebuffer* cur, rtw_features* f_cur,
                          rtw_framebuffer* hist, rtw_features* f_hist, rtw_moments* m_hist, const rtw_reproject_params* p, int moments_history,
                          rtw_framebuffer* dst, rtw_moments* m_dst);
/* The filter.  C, n, z, A, s, EMPTY, BAD, EPS, I_0, h, the tap order and the skip rules are rtw_denoise's; float32 throughout, every product and sum
 * rounded on its own, exp(-e) the hardware exp2.  N = src.accum's count, the history length rtw_reproject* left there; (mu1, mu2) = m.
 * Variance estimate V_0(p), 0 for an empty p:
 *     N >= min_history:   V_0 = max(mu2 - mu1 * mu1, 0)
 *     otherwise           s0 = s1 = s2 = 0
 *                         for dy = -3..3, for dx = -3..3, q = p + (dx, dy)        (in this order)
 *                             skip q when it is outside the frame, empty or bad, or of another shape with RTW_DENOISE_SAME_SHAPE
 *                             e = the normal and depth terms of rtw_denoise with this call's sigmas;  w = exp(-e)      (no h, no colour term)
 *                             s0 += w;  s1 += w * mu1(q);  s2 += w * mu2(q)
 *                         s0 > 0:  a = s1 / s0,  V_0 = max(s2 / s0 - a * a, 0) * ((float)min_history / (float)N);   else V_0 = 0
 * Levels i = 0 .. levels-1, step = 2^i, for every non-empty p:
 *     g(p) = the 3 x 3 prefilter of V_i at distance 1 (not step), dy = -1..1 outer, dx inner, kernel 1/4 centre, 1/8 edges, 1/16 corners;
 *            skip q when it is outside the frame, empty or bad;  g = (sum k * V_i(q)) / (sum k), 0 when no tap counted
 *     the 25 taps of rtw_denoise, whose colour term is replaced by:  if sigma_lum > 0 and p is not bad:
 *            e += |lum(I_i(p)) - lum(I_i(q))| / (sigma_lum * sqrtf(g(p)) + 1e-4f)          (sigma_lum is not halved per level: the variance does that)
 *     the normal and depth terms, w = h[dx] * h[dy] * exp(-e), sw and sc unchanged;  in addition  sv += (w * w) * V_i(q)
 *     I_{i+1}(p) by rtw_denoise's three cases;  V_{i+1}(p) = sv / (sw * sw) when sw > 0, else V_i(p)
 * (The kernels form 1 / (sigma_lum * sqrtf(g) + 1e-4f) once per pixel and multiply, as they do for the depth term.)
 * Output as rtw_denoise: remodulated, dst.accum = (out, count 1), dst.argb the gamma pack.  src, f and m are not written.  With sigma_lum <= 0 the
 * variance plays no part and the result equals rtw_denoise's with sigma_color = 0 and the same other parameters bit for bit.
 * Asynchronous on the context's stream: 1 + levels launches (the estimate includes rtw_denoise's prepare step), levels more with "variance_prefilter" 1.
 * The work space is rtw_denoise's block of the context (52 bytes per pixel, 56 with "variance_prefilter" 1), counted and trimmed with it.
 * "denoise_tiling" applies as for rtw_denoise; neither option changes a bit.
 * RTW_ERR_INVALID: whatever rtw_denoise refuses, a null moments handle, moments of another size or context, min_history outside 1..64. */
typedef struct rtw_denoise_variance_params { int levels; float sigma_lum, sigma_normal, sigma_depth; uint32_t flags; int min_history; } rtw_denoise_variance_params;
/* 5 levels, sigma_lum 4 (a luminance step of four standard deviations costs a factor e), sigma_normal 0.3, sigma_depth 0.1, both flags, min_history 4 */
int rtw_denoise_variance_default_params(rtw_denoise_variance_params* p);
int rtw_denoise_variance(rtw_framebuffer* src, rtw_features* f, rtw_moments* m, const rtw_denoise_variance_params* p, rtw_framebuffer* dst);

/* ---- guided upsampling: a low-resolution frame to full size by its features (joint bilateral upsampling, Kopf et al. 2007; no reference counterpart) ----
 * Render, reproject and filter at a fraction of the frame, then carry the result to full size: the filtered signal is low-frequency (the base colour is
 * divided out), and what is sharp in the final frame -- depth and normal edges, shape boundaries, texture detail -- comes from full-size feature buffers,
 * which are cheap.  It takes buffers and no scene.  lo / f_lo: the low-resolution frame and its features, w x h; f_hi: the features of the same camera at
 * W x H; dst: a W x H framebuffer.  Accepted: w <= W <= 8 w, W * h == H * w (the same aspect, exact in integers), W, H <= 16384; equal sizes are allowed.
 * Everything is float32 unless stated, every product and sum rounded on its own.  C, n, z, A, s, EPS = 1e-3f and the low 30 bits of a shape id are as in
 * rtw_denoise: for a low pixel q they come from lo and f_lo, for a full-size pixel p = (x, y) from f_hi (n_p, z_p, A_p, s_p).  p is EMPTY when f_hi's count
 * is 0: dst.accum = (0, 0, 0, count 0).  q is EMPTY when either of its counts is 0 and BAD when a channel of C_q is not finite.
 * I_q = C_q / (A_q + EPS) with RTW_UPSAMPLE_DEMODULATE, else C_q.
 *  1 tap corner      in integers: the screen point of pixel x of a W-wide frame is (x - W / 2) / W with integer W / 2, as in pixel_dx (no sub-sample offset,
 *                    as in rtw_reproject).  nx = (x - W / 2) * w,  kx = floor(nx / W) (floor division, negative values included),  x0 = kx + w / 2,
 *                    tx = (float)(nx - kx * W) / (float)W; the same for y with H and h.  With equal sizes x0 = x and tx = 0; at an integer ratio every
 *                    ratio-th pixel lands on a low pixel exactly.
 *  2 tap error       e(q) = |n_p - n_q|^2 / sigma_normal^2 + ((z_p - z_q) / (sigma_depth * max(|z_p|, 1e-6)))^2, a term off for a non-positive sigma;
 *                    exp(-e) is the hardware exp2 of -e * log2(e), as in the denoiser.  A tap is SKIPPED when it is outside the low frame, EMPTY or BAD,
 *                    or when RTW_UPSAMPLE_SAME_SHAPE is set and s_q != s_p.  Misses are their own surface.
 *  3 round 1         the taps (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1) in this order, b = (1-tx)(1-ty), tx(1-ty), (1-tx)ty, tx ty; a tap with b == 0
 *                    is skipped.  w = b * exp(-e);  sw += w;  sc += w * I_q.  Accepted when sw >= SW_MIN = 1e-3f: I = sc / sw.
 *  4 round 2         only when round 1 is not accepted (a thin feature or a silhouette that no bilinear tap shows): dy = -1..2 outer, dx = -1..2 inner, the
 *                    taps (x0+dx, y0+dy),  w = k[dx] * k[dy] * exp(-e) with k = (1/8, 3/8, 3/8, 1/8); the same skip rule, the same acceptance.
 *  5 round 3         only when round 2 is not accepted: among the four positions of round 1, the one that is in the frame, not EMPTY and not BAD,
 *                    whatever its shape, with the largest b (the first in order on ties; a position of b == 0 counts here).  I = I_q of that tap.
 *                    None: dst.accum = (0, 0, 0, count 0).
 *  6 output          out = I * (A_p + EPS) with RTW_UPSAMPLE_DEMODULATE, else I;  dst.accum = (out, count 1);  dst.argb = the gamma pack of out; a pixel of
 *                    count 0 packs as black.  dst is then an ordinary one-pass framebuffer for every other call.
 * lo, f_lo and f_hi are not written.  Asynchronous on the context's stream: ONE launch, no work space, no allocation, copy or synchronisation.  The context
 * option "upsample_staging" (-1) picks where the taps are read from -- 0 = global memory, 1 = the tile's box of low-resolution records staged in LDS,
 * -1 = the faster by measurement -- and never changes a bit.
 * RTW_ERR_INVALID, with dst untouched: a null handle or params, a shape outside the rule above, f_lo not of lo's size, dst not of f_hi's size, handles of
 * different contexts, dst == lo, f_lo == f_hi, a NaN sigma, unknown flag bits. */
#define RTW_UPSAMPLE_DEMODULATE 1u
#define RTW_UPSAMPLE_SAME_SHAPE 2u
typedef struct rtw_upsample_params { float sigma_normal, sigma_depth; uint32_t flags; } rtw_upsample_params;
/* sigma_normal 0.3, sigma_depth 0.1 (they mean what they mean in rtw_denoise), both flags */
int rtw_upsample_default_params(rtw_upsample_params* p);
int rtw_upsample(rtw_framebuffer* lo, rtw_features* f_lo, rtw_features* f_hi, const rtw_upsample_params* p, rtw_framebuffer* dst);

/* ---- luminance moments to per-pixel pass budgets: what rtw_render_passes_budget reads (no reference counterpart) ----
 * How many MORE passes each pixel of src should get so that the standard error of its mean luminance falls to `tolerance` of that mean.  It takes buffers
 * and no scene.  N = src.accum's count of the pixel, (mu1, mu2) = m's running means of its luminance and of the square (rtw_reproject_moments).  Every
 * operation is float32 and rounded on its own (no contraction, correctly rounded division); max(a, 0) is fmaxf, so a NaN gives 0.
 *     N < min_history                        b0 = max_passes                        (too short a history to trust the moments)
 *     otherwise                              V = max(mu2 - mu1 * mu1, 0);  d = tolerance * (mu1 + 1e-3f);  need = V / (d * d);  x = need - (float)N
 *         not (x < (float)max_passes)        b0 = max_passes                        (NaN comes here)
 *         else x <= (float)min_passes        b0 = min_passes
 *         else                               b0 = (int)ceilf(x)
 *     budget[p] = the largest b0 among the pixels of the (2 radius + 1)^2 window around p that lie inside the frame   (an edge's neighbours are not starved)
 * src and m are not written.  Asynchronous on the context's stream: ONE launch, no work space, no allocation, copy or synchronisation; budget_dev holds
 * width x height int32, index py * width + px, device memory of the same device.
 * RTW_ERR_INVALID, with budget_dev untouched: a null handle, params or pointer; src and m of different sizes or contexts; tolerance NaN or <= 0;
 * min_passes < 0, max_passes < min_passes or max_passes > 65535; min_history < 1; radius outside 0..2. */
typedef struct rtw_sample_budget_params { float tolerance; int min_history, min_passes, max_passes, radius; } rtw_sample_budget_params;
/* tolerance 0.05, min_history 4, min_passes 0, max_passes 64, radius 1 */
int rtw_sample_budget_default_params(rtw_sample_budget_params* p);
int rtw_sample_budget(rtw_framebuffer* src, rtw_moments* m, const rtw_sample_budget_params* p, void* budget_dev);

/* ---- ambient occlusion from the feature buffers: the tree walk's cheap consumer of a first hit (no reference counterpart) ----
 * How open the surface a pixel shows is: `samples` short rays per pass from the pixel's first hit into the hemisphere of its normal, the share of them
 * (cosine-weighted or not) that reach `radius` unoccluded.  The frame is W x H, shared by f and dst, in the scene's context; the camera is the scene's
 * current camera.  Everything is float32, every product and every sum rounded on its own, in the order written.
 *  1 empty pixels    cf = the int count in f.albedo.w.  A pixel with cf == 0 is EMPTY and is not written.
 *  2 open pixels     z = geom.w / cf;  m = geom.xyz / cf per channel;  n = normalized(m) (tiny vectors are left as they are).  The pixel is OPEN when
 *                    ids.shape < 0 or m.x * m.x + m.y * m.y + m.z * m.z is nearer to 0 than FLT_EPSILON.  An OPEN pixel casts no ray: a = 1 in every pass.
 *  3 ray origin      P = the point the pinhole ray of pixel (x, y) reaches after the distance z (rtw_reproject's step 1: also under a lens);
 *                    O = P + n * bias, per component P.c + n.c * bias.
 *  4 sample rays     for pass k = first_pass .. first_pass + n_passes - 1 and sample s = 0 .. samples - 1:
 *                    key = stream_key(seed, pixel, (k * 64 + s) | 0x40000000) with pixel = y * W + x;  idx = stream_draw31(key, 0) mod RTW_UNIT_TABLE_SIZE;
 *                    v = rtw_unit_table_entry(idx) (no phase, no debug mask);  d = v when dot(v, n) > 0, else reflect(v, n) = v - (n * 2) * dot(v, n).
 *                    The ray is (O, d, radius).  o_s = 1 when rtw_trace_occluded would report it occluded, else 0.
 *                    c_s = max(0, dot(n, d)) with RTW_OCCLUSION_COSINE, else 1;  t_s = o_s ? 0 : c_s.
 *  5 per-pass value  A = t_0 + t_1 + ..., Wt = c_0 + c_1 + ..., both summed left to right from +0;  a = Wt > 0 ? A / Wt : 1.
 *  6 accumulation    per pass, in order: dst.accum.xyz += (a, a, a), count += 1 (AddPixel's shape).  After the call's last pass dst.argb is the gamma
 *                    pack of accum.xyz / count.  Calls accumulate until rtw_framebuffer_clear; dst is an ordinary framebuffer for every other call.
 * The result depends on the scene, the camera, f, the parameters, the passes and the seed only: no option of the context or of the scene changes a bit
 * of it.  The context option "occlusion_order" (-1) picks how the rays are dealt to the lanes -- 0 = a lane per pixel, 1 = a lane per sample, -1 = the
 * faster by measurement.  The whole frame is covered: a rank that rendered only its own feature rows processes only those, by rule 1.
 * f is not written.  Asynchronous on the context's stream: ONE launch whatever n_passes is (the passes loop inside the kernel; a pixel's accumulator entry
 * is read once and written once), no work space, no allocation, copy or synchronisation.  The work counters (rtw_stats) do not count these rays.
 * RTW_ERR_STATE: the scene is not committed.  RTW_ERR_INVALID, with dst untouched: a null handle or params; f and dst of different sizes, or handles of
 * different contexts; samples outside 1..64; radius NaN or <= 0; bias NaN or < 0; unknown flag bits; n_passes < 1; first_pass < 0 or
 * first_pass + n_passes > 2^24. */
#define RTW_OCCLUSION_COSINE 1u
typedef struct rtw_occlusion_params { float radius, bias; int samples; uint32_t flags; } rtw_occlusion_params;
/* radius 1.0, bias 1e-3, samples 8, flags RTW_OCCLUSION_COSINE */
int rtw_occlusion_default_params(rtw_occlusion_params* p);
int rtw_render_occlusion(rtw_scene* scene, rtw_features* f, const rtw_occlusion_params* p, int first_pass, int n_passes, uint32_t seed, rtw_framebuffer* dst);

/* ---- direct lighting from the feature buffers: the reference's point and directional lights, shadowed (Src/Light.h, RayTracerScene::CalculateLightColor,
 * which it ships switched off: USE_LIGHTS 0) ----
 * Per pixel and pass: the sum over up to 8 lights of colour x max(0, n.d) x the unoccluded share of `samples` shadow rays.  The frame is W x H, shared by f
 * and dst, in the scene's context; the camera is the scene's current camera.  Everything is float32, every product and every sum rounded on its own, in the
 * order written.
 *  1 pixel states    EMPTY / OPEN / CAST, the unit normal n, the surface point P and the origin O = P + n * bias: rtw_render_occlusion's steps 1 to 3.  An
 *                    EMPTY pixel is not written.  An OPEN pixel (sky, no usable normal) takes e = (1, 1, 1) in every pass.
 *  2 samples         for pass k = first_pass .. first_pass + n_passes - 1, light j = 0 .. n_lights - 1 and sample s = 0 .. samples - 1:  u = (0, 0, 0) when
 *                    light.radius == 0, else key = stream_key(seed, pixel, (k * 64 + s) | 0xC0000000) with pixel = y * W + x;
 *                    idx = stream_draw31(key, j) mod RTW_UNIT_TABLE_SIZE;  u = rtw_unit_table_entry(idx) (no phase, no debug mask).
 *  3 point light     T = v + u * radius per component;  D = T - O;  dist = sqrt(dot(D, D));  d = D * (1 / dist);  dist == 0 or not finite: c = 0.
 *                    att = 1 / (dist * dist) with RTW_LIGHT_INVERSE_SQUARE, else 1 (the reference has no falloff).
 *  4 directional     v is the direction from the surface towards the light (the reference's PositionOrDirection):  D = v + u * radius;
 *                    d = D * (1 / sqrt(dot(D, D)));  dist = 1000 (the reference's);  att = 1.
 *  5 cosine, cull    c = dot(n, d).  Unless c > 0 (false for a NaN too) t = 0 and NO RAY EXISTS.
 *  6 shadow ray      otherwise the ray is (O, d, dist);  o = 1 where rtw_trace_occluded would report it occluded;  t = o ? 0 : c * att.
 *  7 per light       vis_j = (t_0 + t_1 + ...) / samples, summed left to right from +0.
 *  8 per pass        e += color_j * vis_j per channel, in light order, from +0.  With RTW_LIGHTING_ALBEDO e *= (albedo.xyz / cf) per channel, cf the int
 *                    count in f.albedo.w (the reference's InSurfaceColor * ldp); an OPEN pixel then takes the albedo mean itself: the sky colour.
 *  9 accumulation    per pass, in order: dst.accum.xyz += e, count += 1.  After the call's last pass dst.argb is the gamma pack of accum.xyz / count.  Calls
 *                    accumulate until rtw_framebuffer_clear; dst is an ordinary framebuffer for every other call (rtw_denoise*, rtw_reproject*, rtw_upsample,
 *                    rtw_tonemap, the reads, the resolve and the PNG writer).
 * The result depends on the scene, the camera, f, the lights, the parameters, the passes and the seed only.  The context option "lighting_deal" (-1) picks how
 * the (pixel, light, sample) jobs are dealt to the lanes -- 0 = positional: a lane per pixel, a culled job idles through the walk; 1 = compacted: the jobs that
 * survive step 5 are queued and walked 64 at a time; -1 = the faster by measurement -- and never changes a bit.  Limits: 8 lights, 8 samples, a static scene
 * (the scene as committed), and under a lens P is still the pinhole's point, as for occlusion.
 * `lights` is host memory, copied into the launch's arguments (at most 8 x 36 bytes).  f is not written.  Asynchronous on the context's stream: ONE launch
 * whatever n_passes is (a pixel's accumulator entry is read once and written once), no work space, no allocation, copy or synchronisation.  The work counters
 * (rtw_stats) do not count these rays.
 * RTW_ERR_STATE: the scene is not committed.  RTW_ERR_INVALID, with dst untouched: everything rtw_render_occlusion refuses; n_lights outside 1..8; samples
 * outside 1..8; an unknown type or flag bits; a v, color or radius that is not finite; radius < 0; a directional v whose squared length is not within 1e-3
 * of 1; RTW_LIGHT_INVERSE_SQUARE on a directional light. */
#define RTW_LIGHT_POINT 0
#define RTW_LIGHT_DIRECTIONAL 1
#define RTW_LIGHT_INVERSE_SQUARE 1u          /* per light, point lights only */
typedef struct rtw_light { int type; uint32_t flags; float v[3]; float color[3]; float radius; } rtw_light;
#define RTW_LIGHTING_ALBEDO 1u
typedef struct rtw_lighting_params { float bias; int samples; uint32_t flags; } rtw_lighting_params;
/* bias 1e-3, samples 1, flags RTW_LIGHTING_ALBEDO */
int rtw_lighting_default_params(rtw_lighting_params* p);
int rtw_render_lighting(rtw_scene* scene, rtw_features* f, const rtw_light* lights, int n_lights, const rtw_lighting_params* p, int first_pass, int n_passes, uint32_t seed, rtw_framebuffer* dst);

/* ---- one bounce of indirect light from the feature buffers: what the first hit's neighbourhood, lit by the same lights, sends back to it (no reference
 * counterpart: its path tracer never sees the lights, USE_LIGHTS 0) ----
 * From each pixel's first hit `samples` gather rays go into the scene; the point a ray meets is shaded with the lights and one shadow ray per light, and the
 * radiance comes back weighted by the cosine.  The calls compose by addition: path-traced frame + rtw_render_lighting + rtw_render_indirect.  The frame is
 * W x H, shared by f and dst, in the scene's context; the camera is the scene's current camera.  Everything is float32, every product, sum and quotient
 * rounded on its own, in the order written.
 *  1 pixel states    EMPTY / OPEN / CAST, n, P and O = P + n * bias: rtw_render_occlusion's steps 1 to 3.  An EMPTY pixel is not written.  An OPEN pixel takes
 *                    e = (0, 0, 0) in every pass, and its count still grows: the sky has no indirect term, so direct + indirect does not count the sky twice.
 *  2 gather ray      for pass k and sample s = 0 .. samples - 1 the direction d is exactly the occlusion ray's: the same key (k * 64 + s) |
 *                    RTW_OCCLUSION_STREAM (0x40000000), draw 0, table entry, flipped into n's hemisphere.  c_s = dot(n, d).  The ray is (O, d, 1000).  With
 *                    RTW_INDIRECT_MIRROR d = reflect(w, n) = w - (n * 2) * dot(w, n) instead, w the unit direction of the pixel's pinhole ray; if
 *                    dot(d, n) > 0 is false then, no ray exists and L_s = 0, c_s = 0.
 *  3 gather hit      the closest hit as rtw_trace_closest reports it: shape, position X, normal m.  A miss: L_s is the sky colour of d and no shadow ray is
 *                    cast.  A hit: a_s is the preview colour of that ray, exactly what rtw_render_features records as one sample's albedo (UseBaseColor,
 *                    texel inheritance included, 0 for a shape without material); a Blend in the preview draws from the path stream of step 2's key with its
 *                    counter starting at 1.  O2 = X + m * bias.
 *  4 light jobs      for light j = 0 .. n_lights - 1: rtw_render_lighting's steps 2 to 6 with (O2, m) in place of (O, n), sample index s and counter j of
 *                    the lighting stream, one shadow ray per light: t_j.  E_s = sum_j color_j * t_j, in light order, from +0.  L_s = a_s * E_s per channel.
 *  5 per pass        A = sum_s L_s * c_s per channel, Wt = sum_s c_s, both summed left to right from +0.  g = Wt > 0 ? A / Wt : 0.  With
 *                    RTW_INDIRECT_ALBEDO e = g * (albedo.xyz / cf), otherwise e = g.
 *  6 accumulation    rtw_render_lighting's step 9: dst.accum.xyz += e, count += 1 per pass, the ARGB pack after the call's last pass.
 * The result depends on the scene, the camera, f, the lights, the parameters, the passes and the seed only.  The context option "indirect_deal" (-1) picks how
 * the light jobs of step 4 are dealt to the lanes -- 0 = positional: a job sits where its gather ray sat, a dead one idles through the walk; 1 = compacted: the
 * jobs that survive a miss and the cosine test are queued and walked 64 at a time; -1 = the faster by measurement -- and never changes a bit.  -1 means 1
 * from two light jobs a pixel and pass on (samples x n_lights >= 2) and 0 for one: two sessions on an MI355X measured 1 x 1, 4 x 2 and 8 x 8 samples x
 * lights on two scenes with the default blocks and with the staging blocks below (profiles/indirect_experiments.md).  "indirect_staging" (-1) 1 = 512-thread blocks with a tree's upper levels in LDS where the scene has one to stage, 0 = 256-thread blocks,
 * -1 = by the same sessions 0; it never changes a bit either.
 * Limits: n_lights 0..8, and `lights` may be null when it is 0 (that case gathers the sky alone); samples 1..8; the scene as committed; under a lens the
 * surface point is the pinhole's; emission is not gathered (emitters belong to the path tracer), and an emissive leaf's preview colour is treated like any
 * other preview colour.
 * `lights` is host memory, copied into the launch's arguments.  f is not written.  Asynchronous on the context's stream: ONE launch whatever n_passes is (a
 * pixel's accumulator entry is read once and written once), no work space, no allocation, copy or synchronisation; no ray is stored to memory.  The work
 * counters (rtw_stats) do not count these rays.
 * RTW_ERR_STATE: the scene is not committed.  RTW_ERR_INVALID, with dst untouched: everything rtw_render_lighting refuses, with n_lights outside 0..8
 * (lights null with n_lights > 0) and samples outside 1..8; unknown flag bits. */
#define RTW_INDIRECT_ALBEDO 1u
#define RTW_INDIRECT_MIRROR 2u
typedef struct rtw_indirect_params { float bias; int samples; uint32_t flags; } rtw_indirect_params;
/* bias 1e-3, samples 4, flags RTW_INDIRECT_ALBEDO */
int rtw_indirect_default_params(rtw_indirect_params* p);
int rtw_render_indirect(rtw_scene* scene, rtw_features* f, const rtw_light* lights, int n_lights, const rtw_indirect_params* p, int first_pass, int n_passes, uint32_t seed, rtw_framebuffer* dst);

/* ---- HDR display transform: histogram auto-exposure, a tone curve and the ARGB pack (no reference counterpart: its resolve divides, clamps and packs) ----
 * The chain hands over linear radiance -- emitters, mirror paths onto emitters -- that a clamp to [0, 1] turns white, and a moving camera wants an
 * exposure that follows the frame.  rtw_tonemap meters src with a log-luminance histogram, adapts the exposure of the rtw_exposure object, maps src with
 * the exposure the object held BEFORE the call through a tone curve, and packs ARGB.  It takes buffers and no scene.  Every float product, sum and
 * quotient is float32 and rounded on its own, in the order written; `double` where stated; integers elsewhere.  lum is rtw_denoise_variance's.
 *  1 pixel colour    cnt = src.accum's int count.  A pixel with cnt == 0 is neither counted nor written.  c = sum.xyz / (float)cnt.
 *  2 luminance       L = lum(c) = (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z.
 *  3 bin             the pixel is COUNTED iff L > 0 and L is finite.  u = the bits of L;  bin = clamp((int)(u >> 20) - 856, 0, 255): 8 bins per octave,
 *                    piecewise linear in log2, from 2^-20 to 2^12.  No logarithm is evaluated: h[k] = the number of counted pixels of bin k, exact.
 *  4 new exposure    once, after the whole frame is binned.  N = sum h[k];  N == 0: the object stays as it is (exposure, frames and rtw_exposure_read's
 *                    histogram).  lo = (uint32)((double)low_fraction * N),  hi = (uint32)((double)high_fraction * N);  hi <= lo: lo = 0, hi = N.
 *                    P_k = h[0] + ... + h[k-1];  c_k = |[P_k, P_k + h[k]) n [lo, hi)|;  S = sum k * c_k (64-bit);  in double:
 *                    m = (double)S / (double)(hi - lo),  t = (uint32)((m + 0.5 + 856.0) * 1048576.0) (truncated);  Lavg = the float whose bits are t.
 *                    target = fminf(fmaxf(key / Lavg, min_exposure), max_exposure).
 *                    unmetered object: E = target;  otherwise E = E + (target - E) * adapt.  frames += 1; the object is metered from now on.
 *  5 mapping         E0 = the exposure the object held before this call (1.0f for e == NULL or after create / reset).  x = c * E0 per channel.
 *                    RTW_TONEMAP_LINEAR    y = x
 *                    RTW_TONEMAP_REINHARD  Lx = lum(x);  s = (1.0f + Lx / (white * white)) / (1.0f + Lx) when Lx > 0, else 1.0f;  y = x * s
 *                    RTW_TONEMAP_ACES      per channel v = fmaxf(x, 0.0f);  y = (v * (2.51f * v + 0.03f)) / (v * (2.43f * v + 0.59f) + 0.14f)
 *                    dst.accum = (y, count 1);  dst.argb = the gamma pack of y (rtw_gamma_thresholds, as rtw_denoise writes it): dst is then an
 *                    ordinary one-pass framebuffer for every other call.  dst may be src.
 * The one-frame latency of the exposure is deliberate: the new exposure needs the whole frame's histogram, and mapping with the previous one is what lets
 * a frame be ONE launch that reads each accumulator entry once.  rtw_exposure_meter before the first frame removes it where it matters.
 * With RTW_TONEMAP_HOLD the object's exposure is used and nothing is metered; with e == NULL the exposure is 1 and nothing is metered.
 * Asynchronous on the context's stream: ONE launch, no work space, no allocation, copy or synchronisation.  The context option "tonemap_histogram" (-1)
 * picks how a wave builds its histogram in LDS -- 0 = an atomic per lane, 1 = one addition per distinct bin of the wave's pixels, -1 = the faster by
 * measurement -- and never changes a bit; "tonemap_blocks" (0) > 0 caps the launch's blocks.  One exposure object serves one call at a time.
 * RTW_ERR_INVALID, nothing launched: a null src, params or dst (rtw_exposure_meter: a null e); differing sizes; handles of different contexts; an unknown
 * curve; a NaN parameter; white <= 0; fractions outside 0 <= low_fraction < high_fraction <= 1; min_exposure > max_exposure; adapt outside [0, 1];
 * unknown flag bits; RTW_TONEMAP_HOLD given to rtw_exposure_meter. */
typedef struct rtw_exposure rtw_exposure;       /* device state: the running 256-bin histogram and its ticket, the exposure, the frames metered, the last frame's histogram */
int rtw_exposure_create(rtw_context* ctx, rtw_exposure** out);      /* as after rtw_exposure_reset */
int rtw_exposure_destroy(rtw_exposure* e);
/* unmetered, exposure 1.0f, 0 frames, histogram 0; asynchronous on the context's stream */
int rtw_exposure_reset(rtw_exposure* e);
/* a manual exposure (not NaN): the object counts as metered, so a later metering call adapts from it; frames and histogram stay; asynchronous */
int rtw_exposure_set(rtw_exposure* e, float exposure);
/* waits for the context's stream.  hist256 = the histogram of the LAST metered frame.  Any output may be NULL. */
int rtw_exposure_read(rtw_exposure* e, float* exposure, int32_t* frames, uint32_t hist256[256]);
#define RTW_TONEMAP_LINEAR 0
#define RTW_TONEMAP_REINHARD 1
#define RTW_TONEMAP_ACES 2
#define RTW_TONEMAP_HOLD 1u     /* use the object's exposure, do not meter */
typedef struct rtw_tonemap_params { int curve; float key, white, low_fraction, high_fraction, min_exposure, max_exposure, adapt; uint32_t flags; } rtw_tonemap_params;
/* RTW_TONEMAP_ACES, key 0.18 (the luminance the metered average is brought to), white 4 (Reinhard: the exposed luminance that maps to 1), the pixels
 * between the 50th and the 95th percentile metered, exposure within [1/64, 64], adapt 0.25 (a quarter of the way to the target per frame), no flag */
int rtw_tonemap_default_params(rtw_tonemap_params* p);
/* steps 1 to 4 alone: meters src into e and writes no image */
int rtw_exposure_meter(rtw_framebuffer* src, rtw_exposure* e, const rtw_tonemap_params* p);
int rtw_tonemap(rtw_framebuffer* src, rtw_exposure* e, const rtw_tonemap_params* p, rtw_framebuffer* dst);

/* Device memory the context holds: workspaces + its share of the 201 MB unit-vector table (one copy per device, shared by the contexts on it).
 * The workspace is sized by the largest group of passes rendered (or reserved) so far: per path slot 116 B + 48 B x max_bounce, slots = pixels of the
 * frame's busy tiles x sub-samples x passes per group; e.g. TorusKnot 1080p depth 4: 21 MB for one pass per call,
 * 0.43 GB for a 20-pass call.  When the device has no room for a group's workspace (or it exceeds the option "workspace_limit_mb"), the call renders
 * the same image in smaller groups instead of failing (rtw_context_fallbacks counts how often).  rtw_context_trim gives the workspaces back. */
long long rtw_context_memory_bytes(const rtw_context* ctx);
long long rtw_context_workspace_bytes(const rtw_context* ctx);
int rtw_context_trim(rtw_context* ctx);
int rtw_context_fallbacks(const rtw_context* ctx);

/* ---- multi-GPU: the one exchange of the path.  Every rank renders its own tasks (rtw_render_tasks / rtw_render_passes with rank, world)
 * into a full-size framebuffer; rtw_gather_rows then moves every rank's rows to rank 0 over RCCL (xGMI): one ncclSend / ncclRecv
 * per peer of a compact block of the rank's rows, on the context's stream.  No reference counterpart (the
 * reference is one process); it completes what UpdateBitmapPixels' WaitForAllTasksDone (Src/RayTracerProgram.cpp:303) is to one process.
 * librccl is loaded on first use (dlopen: the library the environment variable RTW_RCCL_LIBRARY names if it is set, else the copy already in the
 * process, e.g. PyTorch's, else librccl.so.1); single-GPU users never load it. ---- */
typedef struct rtw_comm rtw_comm;
#define RTW_COMM_ID_BYTES 128
/* rank 0: a fresh ncclUniqueId, to be handed to every rank by the caller (MPI, torch.distributed, a file ...) */
int rtw_comm_unique_id(uint8_t id[RTW_COMM_ID_BYTES]);
/* every rank: ncclCommInitRank on the context's device */
int rtw_comm_create(rtw_context* ctx, const uint8_t id[RTW_COMM_ID_BYTES], int rank, int world, rtw_comm** out);
/* or: use a communicator the caller already has (an ncclComm_t); it stays the caller's */
int rtw_comm_wrap(rtw_context* ctx, void* nccl_comm, int rank, int world, rtw_comm** out);
int rtw_comm_destroy(rtw_comm* comm);
#define RTW_GATHER_ALL 0        /* accumulator (16 B / pixel) + ARGB (4 B / pixel) */
#define RTW_GATHER_ARGB 1       /* the displayable image only, 4 B / pixel */
/* rows of task t (task_rows rows each, as rtw_render_tasks deals them: t belongs to rank t % world) travel from their owner to rank 0:
 * ONE message per peer -- a sender packs its rows into a compact block (a kernel), the root receives every peer's block inside one RCCL group and
 * unpacks them with one launch; the staging blocks (a rank's share of the frame x 4 or 20 bytes per pixel; the root holds every peer's) are
 * allocated by the first gather of a frame shape.  Asynchronous on the context's stream; every rank of the communicator must call it. */
int rtw_gather_rows(rtw_comm* comm, rtw_framebuffer* fb, int task_rows, int mode);
/* ncclSend / ncclRecv operations this communicator has issued so far (a gather costs a sender one, the root world - 1) */
long long rtw_comm_messages(const rtw_comm* comm);
/* rank 0's *value to every rank (a decision every rank must take alike, e.g. RayTracerProgram::IsTerminating polled on rank 0: a rank that left the
 * progressive loop alone would leave the others blocked in the next gather).  Synchronous; every rank of the communicator must call it. */
int rtw_comm_broadcast_int(rtw_comm* comm, int* value);

/* work counters of launches since the last reset (only counted while enabled) */
int rtw_stats_enable(rtw_context* ctx, int enabled);
int rtw_stats_reset(rtw_context* ctx);
int rtw_stats_get(rtw_context* ctx, rtw_stats* out);

/* tables the device uses, for pinning against the oracle */
uint32_t rtw_rand31(uint32_t seed, uint32_t pixel, uint32_t sample, uint32_t counter);
int rtw_unit_table_entry(uint32_t index, float out3[3]);
int rtw_gamma_thresholds(float out256[256]);
int rtw_texel_lut(float out256[256]);

/* ---- host-side file helpers: RTexture::LoadTexturePNG / SaveBufferToPNG
 * (Src/Texture.cpp:59-199, 201-283) ---- */
int rtw_png_load(const char* path, uint8_t** texels_out, int* width, int* height, int* channels);
void rtw_png_free(uint8_t* texels);
int rtw_png_save_argb(const char* path, const uint32_t* argb, int width, int height);

#ifdef __cplusplus
}
#endif
#endif /* RTWIN_H */
