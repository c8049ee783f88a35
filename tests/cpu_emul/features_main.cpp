// TEST INFRASTRUCTURE: a stand-alone program over the C ABI of include/rtwin.h, linked against the objects of this directory's host build
// (the product's own sources on the HIP stand-in of shim/, AddressSanitizer + UBSan) and run directly -- nothing is preloaded.
// It renders first-hit feature buffers (rtw_render_features) and dumps the three buffers as raw files; tests/test_features_emul.py writes the
// job list and compares the dumps with the model of tests/features_support.py.  It also tries the calls rtw_render_features must refuse.
//
// usage: features_main ASSETS_DIR OUT_DIR JOBS_FILE
// a job line:  name scene pose ex ey ez tx ty tz ux uy uz vfov radius focus traversal width height first_pass n_passes sub_samples task_rows rank world calls
//   scene = torus | mixed (tests/camera_support.py TORUS / MIXED); pose = 0: no camera is ever set, 1: the look-at camera of the line;
//   radius <= 0: no lens; calls = 1: one call of n_passes passes, else n_passes calls of one pass each
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "rtwin.h"

#define CHECK(call) do { const int rc_ = (call); if (rc_ < 0) { std::fprintf(stderr, "features_main: %s -> %d (%s)\n", #call, rc_, rtw_last_error()); return 2; } } while (0)
#define EXPECT(call, want) do { const int rc_ = (call); if (rc_ != (want)) { std::fprintf(stderr, "features_main: %s -> %d, expected %d\n", #call, rc_, (want)); return 2; } } while (0)

static rtw_material_node leaf(int type, float r, float g, float b, float param) { const rtw_material_node n = { type, r, g, b, param, 0, 0, 0 }; return n; }

static int build_scene(rtw_context* ctx, const std::string& which, const std::string& assets, rtw_scene** out)
{
    rtw_scene* s = nullptr;
    CHECK(rtw_scene_create(ctx, &s));
    int idx = -1;
    if (which == "torus") {
        CHECK(rtw_scene_add_mesh_obj(s, (assets + "/TorusKnot.obj").c_str(), &idx));
        const rtw_material_node m = leaf(RTW_MAT_DIFFUSE, 1.0f, 1.0f, 1.0f, 0.0f);
        CHECK(rtw_scene_set_material(s, idx, &m, 1));
    } else if (which == "mixed") {
        const float n[3] = { 0.0f, 1.0f, 0.0f }, p[3] = { 0.0f, -1.2f, 0.0f };
        CHECK(rtw_scene_add_plane(s, n, p, &idx));
        const rtw_material_node ch = leaf(RTW_MAT_DIFFUSE_CHECKER, 0.9f, 0.9f, 0.9f, 2.0f);
        CHECK(rtw_scene_set_material(s, idx, &ch, 1));
        const float c1[3] = { 1.9f, 0.2f, -0.5f };
        CHECK(rtw_scene_add_sphere(s, c1, 0.8f, &idx));
        const rtw_material_node mi = leaf(RTW_MAT_REFLECTIVE, 0.9f, 0.9f, 0.9f, 0.0f);
        CHECK(rtw_scene_set_material(s, idx, &mi, 1));
        const float c2[3] = { -1.9f, -0.3f, 0.6f };
        CHECK(rtw_scene_add_sphere(s, c2, 0.6f, &idx));
        rtw_material_node co[3] = { leaf(RTW_MAT_COMBINE, 0.0f, 0.0f, 0.0f, 0.0f), leaf(RTW_MAT_DIFFUSE, 0.2f, 0.8f, 0.3f, 0.0f), leaf(RTW_MAT_EMISSIVE, 0.3f, 0.1f, 0.1f, 0.0f) };
        co[0].child_a = 1; co[0].child_b = 2;
        CHECK(rtw_scene_set_material(s, idx, co, 3));
        CHECK(rtw_scene_add_mesh_obj(s, (assets + "/BlenderMonkey.obj").c_str(), &idx));
        const rtw_material_node mo = leaf(RTW_MAT_DIFFUSE, 0.9f, 0.8f, 0.7f, 0.0f);
        CHECK(rtw_scene_set_material(s, idx, &mo, 1));
    } else {
        std::fprintf(stderr, "features_main: unknown scene %s\n", which.c_str());
        return 2;
    }
    *out = s;
    return 0;
}

static int dump(const std::string& path, const void* data, size_t bytes)
{
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) { std::fprintf(stderr, "features_main: cannot write %s\n", path.c_str()); return 2; }
    const size_t n = std::fwrite(data, 1, bytes, f);
    std::fclose(f);
    return n == bytes ? 0 : 2;
}

// the calls rtw_render_features must refuse, each with its status; none of them may touch a buffer
static int refusals(rtw_context* ctx, const std::string& assets)
{
    rtw_scene* scene = nullptr;
    if (build_scene(ctx, "torus", assets, &scene) != 0) return 2;
    rtw_features* f = nullptr;
    EXPECT(rtw_features_create(ctx, 0, 8, &f), RTW_ERR_INVALID);
    EXPECT(rtw_features_create(ctx, 8, -1, &f), RTW_ERR_INVALID);
    EXPECT(rtw_features_create(nullptr, 8, 8, &f), RTW_ERR_INVALID);
    EXPECT(rtw_features_wrap(ctx, 8, 8, nullptr, nullptr, nullptr, &f), RTW_ERR_INVALID);
    CHECK(rtw_features_create(ctx, 16, 8, &f));
    EXPECT(rtw_render_features(scene, f, 10, 0, 1, 0, 1, 2, 1u), RTW_ERR_STATE);          // not committed
    CHECK(rtw_scene_commit(scene));
    EXPECT(rtw_render_features(nullptr, f, 10, 0, 1, 0, 1, 2, 1u), RTW_ERR_INVALID);
    EXPECT(rtw_render_features(scene, nullptr, 10, 0, 1, 0, 1, 2, 1u), RTW_ERR_INVALID);
    EXPECT(rtw_render_features(scene, f, 0, 0, 1, 0, 1, 2, 1u), RTW_ERR_INVALID);         // task_rows
    EXPECT(rtw_render_features(scene, f, 10, 2, 2, 0, 1, 2, 1u), RTW_ERR_INVALID);        // rank >= world
    EXPECT(rtw_render_features(scene, f, 10, 0, 0, 0, 1, 2, 1u), RTW_ERR_INVALID);        // world
    EXPECT(rtw_render_features(scene, f, 10, 0, 1, -1, 1, 2, 1u), RTW_ERR_INVALID);       // first_pass
    EXPECT(rtw_render_features(scene, f, 10, 0, 1, 0, -1, 2, 1u), RTW_ERR_INVALID);       // n_passes
    EXPECT(rtw_render_features(scene, f, 10, 0, 1, 0, 1, 0, 1u), RTW_ERR_INVALID);        // sub_samples
    EXPECT(rtw_render_features(scene, f, 10, 0, 1, 0, 1, 5, 1u), RTW_ERR_INVALID);
    rtw_context* other = nullptr;
    CHECK(rtw_context_create(0, &other));
    rtw_features* foreign = nullptr;
    CHECK(rtw_features_create(other, 16, 8, &foreign));
    EXPECT(rtw_render_features(scene, foreign, 10, 0, 1, 0, 1, 2, 1u), RTW_ERR_INVALID);  // another context's buffers
    CHECK(rtw_features_destroy(foreign));
    CHECK(rtw_context_destroy(other));
    EXPECT(rtw_render_features(scene, f, 10, 0, 1, 1 << 29, 1, 2, 1u), RTW_OK);           // no lens: no limit on the pass index
    CHECK(rtw_features_clear(f));
    const rtw_lens lens = { 0.1f, 5.0f };
    CHECK(rtw_scene_set_lens(scene, &lens));
    EXPECT(rtw_render_features(scene, f, 10, 0, 1, 1 << 29, 1, 2, 1u), RTW_ERR_LIMIT);
    EXPECT(rtw_render_features(scene, f, 10, 0, 1, (1 << 29) - 1, 2, 2, 1u), RTW_ERR_LIMIT);
    EXPECT(rtw_render_features(scene, f, 10, 0, 1, 0, 0, 2, 1u), RTW_OK);                 // no pass: nothing happens
    // every refused call left the cleared buffers alone
    std::vector<float> geom(16 * 8 * 4), albedo(16 * 8 * 4);
    std::vector<int32_t> ids(16 * 8 * 2);
    CHECK(rtw_features_read(f, geom.data(), albedo.data(), ids.data()));
    for (float v : geom) if (v != 0.0f) { std::fprintf(stderr, "features_main: a refused call wrote geom\n"); return 2; }
    for (float v : albedo) if (v != 0.0f) { std::fprintf(stderr, "features_main: a refused call wrote albedo\n"); return 2; }
    for (int32_t v : ids) if (v != -1) { std::fprintf(stderr, "features_main: a refused call wrote ids\n"); return 2; }
    void *g = nullptr, *a = nullptr, *i = nullptr;
    CHECK(rtw_features_device_pointers(f, &g, &a, &i));
    if (!g || !a || !i) { std::fprintf(stderr, "features_main: null device pointers\n"); return 2; }
    CHECK(rtw_features_read(f, nullptr, nullptr, nullptr));
    CHECK(rtw_features_destroy(f));
    CHECK(rtw_scene_destroy(scene));
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 4) { std::fprintf(stderr, "usage: features_main ASSETS_DIR OUT_DIR JOBS_FILE\n"); return 2; }
    const std::string assets = argv[1], outdir = argv[2];
    FILE* jobs = std::fopen(argv[3], "r");
    if (!jobs) { std::fprintf(stderr, "features_main: cannot read %s\n", argv[3]); return 2; }
    rtw_context* ctx = nullptr;
    CHECK(rtw_context_create(0, &ctx));
    CHECK(rtw_stats_enable(ctx, 1));
    CHECK(rtw_stats_reset(ctx));
    char name[96], scene_name[32];
    float e[3], t[3], u[3], vfov, radius, focus;
    int pose, traversal, W, H, first_pass, n_passes, ns, task_rows, rank, world, calls, done = 0;
    while (std::fscanf(jobs, "%95s %31s %d %f %f %f %f %f %f %f %f %f %f %f %f %d %d %d %d %d %d %d %d %d %d", name, scene_name, &pose, &e[0], &e[1], &e[2],
                       &t[0], &t[1], &t[2], &u[0], &u[1], &u[2], &vfov, &radius, &focus, &traversal, &W, &H, &first_pass, &n_passes, &ns, &task_rows, &rank, &world, &calls) == 25) {
        rtw_scene* scene = nullptr;
        if (build_scene(ctx, scene_name, assets, &scene) != 0) return 2;
        if (pose) {
            rtw_camera cam;
            CHECK(rtw_camera_look_at(e, t, u, vfov, &cam));
            CHECK(rtw_scene_set_camera(scene, &cam));
        }
        CHECK(rtw_scene_commit(scene));
        CHECK(rtw_scene_set_traversal(scene, traversal));
        if (radius > 0.0f) {
            const rtw_lens lens = { radius, focus };
            CHECK(rtw_scene_set_lens(scene, &lens));
        }
        rtw_features* f = nullptr;
        CHECK(rtw_features_create(ctx, W, H, &f));
        if (calls == 1) CHECK(rtw_render_features(scene, f, task_rows, rank, world, first_pass, n_passes, ns, 12345u));
        else for (int k = 0; k < n_passes; k++) CHECK(rtw_render_features(scene, f, task_rows, rank, world, first_pass + k, 1, ns, 12345u));
        std::vector<float> geom((size_t)W * H * 4), albedo((size_t)W * H * 4);
        std::vector<int32_t> ids((size_t)W * H * 2);
        CHECK(rtw_features_read(f, geom.data(), albedo.data(), ids.data()));
        if (dump(outdir + "/" + name + ".geom", geom.data(), geom.size() * 4) || dump(outdir + "/" + name + ".albedo", albedo.data(), albedo.size() * 4) ||
            dump(outdir + "/" + name + ".ids", ids.data(), ids.size() * 4)) return 2;
        CHECK(rtw_features_destroy(f));
        CHECK(rtw_scene_destroy(scene));
        done++;
    }
    std::fclose(jobs);
    // rtw_stats is not touched by feature calls, counting switched on or not
    rtw_stats st;
    CHECK(rtw_stats_get(ctx, &st));
    if (st.rays || st.box_tests || st.tri_tests || st.shaded_hits || st.tex_samples || st.camera_rays) { std::fprintf(stderr, "features_main: a feature call moved the work counters\n"); return 2; }
    CHECK(rtw_stats_enable(ctx, 0));
    if (refusals(ctx, assets) != 0) return 2;
    CHECK(rtw_context_destroy(ctx));
    std::printf("features_main ok: %d frames, refusals checked\n", done);
    return 0;
}
