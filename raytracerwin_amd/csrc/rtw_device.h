// rtw_device.h -- launch wrappers implemented in rtw_device.hip (internal).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <climits>

#include "rtw_types.h"

#define RTW_MAX_BOUNCE_DEV 16

namespace rtw {

// bytes of level workspace a launch of `work_items` threads needs (rounded up to whole 256-thread blocks)
inline size_t level_workspace_bytes(long long work_items, int max_bounce)
{
    const size_t threads = (size_t)((work_items + 255) / 256) * 256;
    return threads * (size_t)(max_bounce > 0 ? max_bounce : 1) * 3 * 16;
}
struct PipelineLayout { size_t queue_off, pend_off, counters_off, rad_off, hit_off, state_off, tlist0_off, tlist1_off, ws_off, total, capacity; };
// workspace of the bins + wave pipeline (pipeline 3) for a launch of `work_items` pixels (device bytes)
size_t pipeline_workspace_bytes(long long work_items, int max_bounce, PipelineLayout* out);
// Sky-only tiles are rendered by a kernel of their own on aux_stream, between the two events (fork after the previous work of the main stream, join
// before the pass or group ends); aux_stream null = on the main stream.  A run of passes inside one rtw_render_passes call forks the second stream before
// its first pass and joins it after its last: between those passes nothing else can be enqueued, the sky kernels are ordered on their own stream and
// write pixels no other kernel of the run writes.
struct AuxFork {
    hipStream_t aux_stream = nullptr; hipEvent_t fork_event = nullptr, join_event = nullptr;
    bool do_fork = true, do_join = true;
    bool* aux_unjoined = nullptr;   // set when a sky kernel was launched and the join was left to a later pass
};
struct PipelineTuning : AuxFork {
    int expected_paths;    // queue length seen by the previous pass on this context, -1 = unknown
    int round_hint[32];    // trace-list lengths of the previous pass per round, -1 = unknown
    int sky_job0; const float* gamma_thr;   // jobs [sky_job0, n_jobs) of the job table are sky-only tiles, rendered by primary_sky_kernel
    bool has_analytic = false;  // some shape is a sphere / plane / capsule: the kernels' instantiations that hold those tests are launched
    bool skip_trace = false;    // every shape is a leading analytic shape: the shading lanes do the whole scene query, no trace launches
    bool counters_clean;   // the counters are known to be zero (left so by the previous pass): no memset
    int cu_count;
    hipEvent_t* timing;    // null, or 4 events recorded before the primary kernel and after each of the three stages
};
int launch_render_pipeline(const RtwSceneDev* sc, void* accum, void* argb, void* workspace, const RtwRenderParams& p, const PipelineTuning& tune, bool stats, hipStream_t stream);
// ---- pass-batched pipeline (pipeline 4, rtw_group_kernels.h) ----
// slots of a group's workspace (rtw_group_kernels.h group_slot): one per path and pass
inline size_t group_capacity(size_t paths_per_pass, int n_passes) { return paths_per_pass * (size_t)(n_passes > 0 ? n_passes : 1); }
struct GroupLayout { size_t counters_off, rad_off, state_off, hit_off, carry_off, levels_off, list0_off, list1_off, overflow_off, tlist0_off, tlist1_off, total; };
// device bytes of a group's workspace: `capacity` path slots (busy tiles x 64 x sub-samples x passes of the group, rounded up to a power of two of passes)
size_t group_workspace_bytes(size_t capacity, int max_bounce, bool carry, GroupLayout* out);
// The material class of a launch (== RTW_MATERIAL_CLASS_* of rtwin.h): which instantiation of gprimary_kernel / gshade_kernel it runs.
//   GENERAL   the whole material machine: tree walk, evaluation stack, Blend's draw, fuzzy Reflective's double-precision transcendentals, texels
//   FLAT      every material tree of the scene is ONE node, Diffuse or Checker, and no mesh has a valid texture: the leaf is evaluated directly, a hit's
//             sampled colour is exactly (1, 1, 1) with alpha 1, nothing is emitted -- fields 1 and 2 of a level are never written or read
//   FLAT_TEX  the same trees, some mesh textured: the texel sample and the transparent-texel branch stay
#define RTW_MC_GENERAL 0
#define RTW_MC_FLAT 1
#define RTW_MC_FLAT_TEX 2
struct GroupTuning : AuxFork {      // (the sky-only tiles run on aux_stream beside the rest of the group)
    size_t capacity = 0;
    int material_class = RTW_MC_GENERAL;   // the caller asks for a flat class only where its instantiations exist: no analytic shape, no lens, no work counters
    const float* gamma_thr = nullptr;
    bool has_analytic = false;     // some shape is a sphere / plane / capsule / triangle
    bool carry = false;            // ... and one of them follows a textured mesh: hit records carry the mesh hit whose texel the hit keeps
    bool counters_clean = false;   // the list counters are zero (left so by the previous group)
    int round_hint[32];            // list lengths of the previous group per round (-1 = unknown): they size the launches
    int cu_count = 256;
    int staged_shape = -1, staged_top = 0;   // the trace blocks stage the first staged_top tnodes records of this shape in LDS (-1: nothing staged)
    bool staged_all = false;                 // ... and that is the shape's whole tree
    bool staged_planes = false;              // ... and the triangles' planes are staged beside it (persistent kernel: back-facing leaves are never noted)
    int staged_tris = 0;                     // triangles of the staged shape
    bool single_mesh = false;      // the scene is one mesh: the trace rounds run persistent waves that refill their lanes
    bool lead_mesh = false;        // ... or leading analytic shapes followed by ONE mesh (shape staged_shape), no texel inheritance: the same kernel, continuing the lead query
    // a group rendered as several parts on as many streams (rtwin_capi.cpp: rtw_render_passes): the group's sky tiles are rendered for ALL its passes
    // (sky_first_pass, sky_passes) by one launch enqueued ahead of the parts (sky_mode 2); a part's resolve kernel waits for the previous part's
    // (resolve_after) and signals the next (resolve_done)
    int sky_blocks = 4;  // blocks of the sky kernel per CU at most (its lanes loop over the tiles)
    int sky_passes = 0, sky_first_pass = 0, sky_mode = 0; hipEvent_t resolve_after = nullptr, resolve_done = nullptr;       // sky_mode 0: a whole group (sky on aux_stream beside it), 1: a part of a split group (no sky tiles), 2: ONLY the sky tiles of a split group, all its passes
    int visit_budget = INT32_MAX;            // persistent trace waves: a ray that needs more node visits than this is handed to a wave-per-ray launch that follows
    int trace_hint[32];                      // scenes with leading analytic shapes: how many rays of a round still went to the trace launch (previous group)
    bool skip_trace = false;                 // every shape is a leading analytic shape: the shading lanes do the whole query, no trace launches
    int overflow_hint[32];                   // how many rays that were in the previous group, per round (-1 = unknown)
    int wave_below = 0;                      // a trace round whose list (previous group's length) is shorter than this runs a wave per ray
    bool camera_round = false;               // a lens (rp.lens): glens_kernel makes the camera rays and the trace kernels find their hits in a round of its own
                                             // ahead of the bounce rounds; false: gprimary_kernel's LENS instantiation walks the trees itself (option "lens_route")
    hipEvent_t* timing = nullptr;  // null, or 4 events: before the primary kernel, after it, after the bounce rounds, after resolve
};
int material_class_of_launch(int scene_class, bool stats, bool has_analytic, bool lens);      // the class launch_render_group instantiates its shade / primary kernels for
int launch_render_group(const RtwSceneDev* sc, void* accum, void* argb, void* workspace, const RtwGroupParams& g, const GroupTuning& tune, bool stats, hipStream_t stream);
// ---- first-hit feature buffers (rtw_feature_kernels.h): g holds the frame, the tile mapping and the busy / sky tile lists of a group launch (rp.preview and
// rp.max_bounce are not read); geom / albedo: float4 per pixel, ids: int32 x 2 per pixel ----
struct FeatureTuning {
    int cu_count = 256, sky_blocks = 4;
    bool has_analytic = false;     // some shape is a sphere / plane / capsule / triangle
    bool carry = false;            // ... and one of them follows a textured mesh: its hits can keep that mesh hit's sampled colour
};
int launch_render_features(const RtwSceneDev* sc, void* geom, void* albedo, void* ids, const RtwGroupParams& g, const FeatureTuning& tune, hipStream_t stream);
// ---- the a-trous denoiser over a framebuffer and its feature buffers (rtw_denoise_kernels.h): prepare, then `levels` level launches ping-ponging
// between the workspace's two images, the last one writing dst.  Nothing but launches on `stream`. ----
constexpr uint32_t DENOISE_DEMODULATE = 1u, DENOISE_SAME_SHAPE = 2u;      // == RTW_DENOISE_* of rtwin.h
struct DenoiseCall {
    const void *accum, *geom, *albedo, *ids;    // the sources (never written)
    void* workspace;                            // denoise_workspace_bytes(width, height)
    void *dst_accum, *dst_argb;
    const float* gamma_thr;
    int width, height, levels;
    float sigma_color, sigma_normal, sigma_depth;
    uint32_t flags;
    int tiling;                                 // per level: 0 = dense, 1 = lattice, -1 = the measured rule (denoise_level_is_lattice)
};
size_t denoise_workspace_bytes(int width, int height);     // two float4 images + the guide records (16 + 4 bytes): 52 bytes per pixel
bool denoise_level_is_lattice(int tiling, int step);
int launch_denoise(const DenoiseCall& d, hipStream_t stream);
// ---- temporal reprojection of a history frame into the current one (rtw_reproject_kernels.h): one launch on `stream`, no workspace ----
constexpr uint32_t REPROJECT_DEMODULATE = 1u;       // == RTW_REPROJECT_DEMODULATE of rtwin.h
struct ReprojectCall {
    const void *cur_accum, *cur_geom, *cur_albedo, *cur_ids;        // the current frame and the history with its features (never written)
    const void *hist_accum, *hist_geom, *hist_albedo, *hist_ids;
    void *dst_accum, *dst_argb;
    const float* gamma_thr;
    RtwCamera cam_cur, cam_prev;
    int width, height, max_history;
    float depth_tolerance, normal_cos;
    uint32_t flags;
    int staging;                                // 0 = taps from global memory, 1 = the block's tap box staged in LDS, -1 = the measured rule (reproject_is_staged)
};
bool reproject_is_staged(int staging, const RtwCamera& cur, const RtwCamera& prev);
int launch_reproject(const ReprojectCall& r, hipStream_t stream);
// ... with luminance moments (rtw_reproject_moments): the same call, the moments variant of the kernel; still one launch.  All three pointers set.
struct ReprojectMomentsCall { const void* hist; void* dst; int history; };     // float2 (mu1, mu2) per pixel; moments_history
int launch_reproject_moments(const ReprojectCall& r, const ReprojectMomentsCall& m, hipStream_t stream);
// ---- guided upsampling of a low-resolution framebuffer under full-size features (rtw_upsample_kernels.h): one launch on `stream`, no workspace ----
constexpr uint32_t UPSAMPLE_DEMODULATE = 1u, UPSAMPLE_SAME_SHAPE = 2u;    // == RTW_UPSAMPLE_* of rtwin.h
struct UpsampleCall {
    const void *lo_accum, *lo_geom, *lo_albedo, *lo_ids;            // the low-resolution frame and its features (never written)
    const void *hi_geom, *hi_albedo, *hi_ids;                       // the full-size features (never written)
    void *dst_accum, *dst_argb;
    const float* gamma_thr;
    int width, height, lo_width, lo_height;     // lo_width <= width <= 8 lo_width, width * lo_height == height * lo_width, width and height <= 16384
    float sigma_normal, sigma_depth;
    uint32_t flags;
    int staging;                                // 0 = taps from global memory, 1 = the tile's box of low-resolution records staged in LDS, -1 = the measured rule (upsample_is_staged)
};
bool upsample_is_staged(int staging);
int launch_upsample(const UpsampleCall& u, hipStream_t stream);
// ---- luminance moments -> per-pixel pass budgets (rtw_budget_kernels.h): one launch on `stream`, no workspace ----
struct SampleBudgetCall {
    const void *accum, *moments;                // float4 (sum rgb, int count) and float2 (mu1, mu2) per pixel (never written)
    void* budget;                               // int32 per pixel
    int width, height;
    float tolerance;
    int min_history, min_passes, max_passes, radius;    // radius 0..2
};
int launch_sample_budget(const SampleBudgetCall& s, hipStream_t stream);
// ---- the variance-guided a-trous filter (rtw_variance_kernels.h): the estimate (prepare included), then `levels` level launches -- each preceded by a
// prefilter launch when prefilter_pass is set -- ping-ponging between the workspace's two images, the last one writing dst ----
struct DenoiseVarianceCall {
    const void *accum, *geom, *albedo, *ids, *moments;      // the sources (never written)
    void* workspace;                            // denoise_variance_workspace_bytes(width, height, prefilter_pass)
    void *dst_accum, *dst_argb;
    const float* gamma_thr;
    int width, height, levels, min_history;
    float sigma_lum, sigma_normal, sigma_depth;
    uint32_t flags;
    int tiling;                                 // as DenoiseCall's
    bool prefilter_pass;                        // g(p) from a pass of its own (true) or fetched by the level kernels (false): denoise_variance_prefilter_is_pass
};
size_t denoise_variance_workspace_bytes(int width, int height, bool prefilter_pass);     // rtw_denoise's 52 bytes per pixel, + 4 with the prefilter pass
bool denoise_variance_prefilter_is_pass(int option);
int launch_denoise_variance(const DenoiseVarianceCall& d, hipStream_t stream);
// ---- KdNode::Build and the layouts derived from the tree, on the device (rtw_build_kernels.h) ----
struct DeviceBuildIn {      // the arrays RMeshShape owns (host memory)
    const float* points; int n_points; const float* texcoords; int n_texcoords; const float* normals; int n_normals;
    const int32_t* idx_p; const int32_t* idx_t; const int32_t* idx_n; const int32_t* tri_material; int n_tris;
};
struct DeviceBuildOut {     // device memory, the caller's from here on (hipFree)
    RtwNode* nodes; RtwPNode* tnodes; RtwTri* tris; RtwShade* shade; float* flat[3];
    int n_nodes, tnodes_top, max_depth, flat_n[3], flat_pad[3];
};
int device_build_mesh(const DeviceBuildIn& in, int top_budget, DeviceBuildOut* out, hipStream_t stream);
int device_build_bins(const RtwNode* d_nodes, const RtwTri* d_tris, int n_nodes, const RtwCamera& cam, int width, int height, int bin_w, int bin_h,
                      uint32_t** off_out, uint32_t** ent_out, uint32_t* h_off, int* has_bins, hipStream_t stream);
#define RTW_PERSIST_CAND_BYTES (8 * 1024 * 4)   // candidate lists of a persistent trace block: RTW_GT_CAP_STAGED words x 1024 threads
#define RTW_TNODES_TOP_BUDGET 3072 // records (32 B each) of a tree's upper levels a block of the ray-per-lane trace kernel stages in LDS: 96 KiB
int launch_render(const RtwSceneDev* sc, void* accum, void* argb, void* ws, const RtwRenderParams& p, bool stats, hipStream_t stream);
int launch_closest(const RtwSceneDev* sc, const float* rays, long long n, float* hits11, int* shape, int* tri, bool stats, hipStream_t stream);
// ---- ray queries on the caller's device buffers (rtw_query_kernels.h) ----
struct QueryTuning {
    int cu_count = 256;
    int blocks = 0;                          // > 0: at most exactly this many blocks (option "query_blocks"); 0: cu_count x blocks per CU
    bool single_mesh = false;                // the scene is one mesh: the instantiation without the analytic tests
    bool carry = false;                      // an analytic shape follows a textured mesh: its hits can keep that mesh hit's sampled colour
    int staged_shape = -1, staged_top = 0;   // as GroupTuning: the first mesh whose upper tree levels a block stages in LDS
    bool staged_all = false;
};
void query_launch_shape(const QueryTuning& q, long long n, int* threads, unsigned* blocks);
int launch_shape_to_byte(const int* shape, long long n, uint8_t* out, hipStream_t stream);       // out[i] = shape[i] >= 0
int launch_query(const RtwSceneDev* sc, const float* rays, long long n, float* hits11, int* shape, int* tri, uint8_t* occluded, const QueryTuning& q, bool stats, hipStream_t stream);
// ---- ambient occlusion from the feature buffers (rtw_occlusion_kernels.h): one launch on `stream`, no workspace ----
constexpr uint32_t OCCLUSION_COSINE = 1u;       // == RTW_OCCLUSION_COSINE of rtwin.h
struct OcclusionCall {
    const void *geom, *albedo, *ids;            // the features (never written)
    void *accum, *argb;                         // the destination: accumulated into
    const float* gamma_thr;
    RtwCamera cam;
    int width, height;
    float radius, bias;
    int samples;                                // 1..64
    uint32_t flags;
    int first_pass, n_passes;
    uint32_t seed;
    int order;                                  // 0 = a lane per pixel, 1 = a lane per sample, -1 = the measured rule (occlusion_is_by_sample)
    int cu_count = 256;
    bool single_mesh = false;                   // as QueryTuning's
    int staged_shape = -1, staged_top = 0;
    bool staged_all = false;
};
bool occlusion_is_by_sample(int order);
void occlusion_launch_shape(const OcclusionCall& o, int* threads, unsigned* blocks, int* staged_top, bool* staged_all);
int launch_occlusion(const RtwSceneDev* sc, const OcclusionCall& o, hipStream_t stream);
// ---- direct lighting from the feature buffers (rtw_lighting_kernels.h): one launch on `stream`, no workspace; the lights travel in the launch's arguments ----
constexpr uint32_t LIGHTING_ALBEDO = 1u;        // == RTW_LIGHTING_ALBEDO of rtwin.h
struct LightingCall {
    const void *geom, *albedo, *ids;            // the features (never written)
    void *accum, *argb;                         // the destination: accumulated into
    const float* gamma_thr;
    RtwCamera cam;
    int width, height;
    RtwLight lights[RTW_LT_MAX];
    int n_lights;                               // 1..RTW_LT_MAX
    float bias;
    int samples;                                // 1..RTW_LT_MAX
    uint32_t flags;
    int first_pass, n_passes;
    uint32_t seed;
    int deal;                                   // 0 = positional, 1 = compacted, -1 = the measured rule (lighting_is_compacted)
    int cu_count = 256;
    bool single_mesh = false;                   // as QueryTuning's
    int staged_shape = -1, staged_top = 0;
    bool staged_all = false;
};
bool lighting_is_compacted(int deal);
void lighting_launch_shape(const LightingCall& o, int* threads, unsigned* blocks, int* staged_top, bool* staged_all);
int launch_lighting(const RtwSceneDev* sc, const LightingCall& o, hipStream_t stream);
// ---- one bounce of indirect light from the feature buffers (rtw_indirect_kernels.h): one launch on `stream`, no workspace ----
constexpr uint32_t INDIRECT_ALBEDO = 1u, INDIRECT_MIRROR = 2u;     // == RTW_INDIRECT_* of rtwin.h
struct IndirectCall {
    const void *geom, *albedo, *ids;            // the features (never written)
    void *accum, *argb;                         // the destination: accumulated into
    const float* gamma_thr;
    RtwCamera cam;
    int width, height;
    RtwLight lights[RTW_LT_MAX];
    int n_lights;                               // 0..RTW_LT_MAX
    float bias;
    int samples;                                // 1..RTW_LT_MAX
    uint32_t flags;
    int first_pass, n_passes;
    uint32_t seed;
    int deal;                                   // 0 = positional, 1 = compacted, -1 = the rule (indirect_is_compacted)
    int staging = -1;                           // 1 = staging blocks of 512 threads, 0 = nothing staged (256-thread blocks), -1 = the rule (indirect_is_staged)
    int cu_count = 256;
    bool single_mesh = false, carry = false;    // as QueryTuning's
    int staged_shape = -1, staged_top = 0;
    bool staged_all = false;
};
bool indirect_is_compacted(int deal, int samples, int n_lights);
bool indirect_is_staged(int staging);
void indirect_launch_shape(const IndirectCall& o, int* threads, unsigned* blocks, int* staged_top, bool* staged_all);
int launch_indirect(const RtwSceneDev* sc, const IndirectCall& o, hipStream_t stream);
// ---- the HDR display transform (rtw_tonemap_kernels.h): histogram metering, exposure, tone curve and pack in one launch on `stream`, no workspace ----
constexpr int TONEMAP_LINEAR = 0, TONEMAP_REINHARD = 1, TONEMAP_ACES = 2;      // == RTW_TONEMAP_* of rtwin.h
constexpr int TONEMAP_BIN0 = 856;               // bin = (float bits >> 20) - 856: 8 bins per octave from 2^-20
// the 32-bit words of an exposure object's device state
constexpr int EXPOSURE_HIST = 0;                // 256: the running launch's histogram; zero between launches
constexpr int EXPOSURE_LAST = 256;              // 256: the histogram of the last metered frame
constexpr int EXPOSURE_TICKET = 512;            // blocks of the running launch that have filed their bins; zero between launches
constexpr int EXPOSURE_VALUE = 513;             // the exposure's float bits
constexpr int EXPOSURE_METERED = 514;           // 0 until a frame was metered or an exposure set
constexpr int EXPOSURE_FRAMES = 515;            // frames metered
constexpr int EXPOSURE_WORDS = 516;
struct TonemapCall {
    const void* src_accum;
    void *dst_accum, *dst_argb;                 // null for meter-only (write false); may be the source's
    const float* gamma_thr;
    uint32_t* state;                            // the exposure object's words; null: exposure 1, no metering
    int width, height, curve;
    float key, white, low_fraction, high_fraction, min_exposure, max_exposure, adapt;
    bool meter, write;
    int histogram;                              // 0 = an LDS atomic per lane, 1 = wave-aggregated, -1 = the measured rule (tonemap_histogram_is_aggregated)
    int cu_count = 256;
    int blocks = 0;                             // > 0: at most this many blocks (option "tonemap_blocks")
};
bool tonemap_histogram_is_aggregated(int option);
unsigned tonemap_blocks(const TonemapCall& c);
int launch_tonemap(const TonemapCall& c, hipStream_t stream);
int launch_exposure_state(uint32_t* state, float exposure, bool metered, bool clear, hipStream_t stream);
int launch_ray_trace(const RtwSceneDev* sc, const float* rays, const uint32_t* keys2, long long n, int max_bounce, int preview,
                     uint32_t seed, unsigned long long npix, float* rgb, void* ws, bool stats, hipStream_t stream);
int launch_texture_sample(const RtwSceneDev* sc, int shape, int mat, const float* uv, long long n, float* rgba, hipStream_t stream);
// ---- multi-GPU gather (rtw_gather_rows): every rank's task rows travel as ONE compact block per rank -- [ARGB of its pixels in task order |
// their accumulators] -- packed by the sender, unpacked into the framebuffer by the root, all peers in one launch ----
struct GatherBlocks { int n = 0, first_rank = 0; uint64_t off[64]; uint32_t px[64]; };     // blocks of ranks first_rank .. first_rank + n - 1 inside the staging buffer
size_t gather_block_bytes(size_t pixels, bool with_accum);
int launch_gather_rows(bool unpack, void* argb, void* accum, void* stage, int width, int task_rows, int world, const GatherBlocks& b, bool with_accum, hipStream_t stream);

}  // namespace rtw
