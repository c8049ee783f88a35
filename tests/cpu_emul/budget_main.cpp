// TEST INFRASTRUCTURE: a stand-alone program over the C ABI of include/rtwin.h, linked against the objects of this directory's host build
// (the product's own sources on the HIP stand-in of shim/, AddressSanitizer + UBSan) and run directly -- nothing is preloaded.
// Per job it renders a 40 x 21 frame that already holds two passes: the six uniform snapshots k = 0..5 of passes 3.. (rtw_render_passes) and ONE
// budgeted call (rtw_render_passes_budget, 5 passes) under the budgets of DIR/budget.i32, each from the same starting frame, and dumps accumulator and
// ARGB words as raw files; then rtw_sample_budget at radius 2 over DIR/sb_accum.f32 and DIR/sb_mu.f32 into DIR/sb.i32.  tests/test_budget_emul.py
// writes the inputs and compares the dumps.  On the stand-in device memory is host memory: the buffers are plain vectors, wrapped.
//
// usage: budget_main ASSETS_DIR DIR        (DIR/jobs.txt: a job a line)
// a job line:    name scene_file sub_samples group_max split_paths split_min      (the three options hold for the budgeted call only)
// a scene line:  sphere cx cy cz r NODES | plane nx ny nz px py pz NODES | capsule sx sy sz ex ey ez r NODES | mesh NAME NODES
//                NODES: a file of rtw_material_node records (32 bytes each)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rtwin.h"

#define CHECK(call) do { const int rc_ = (call); if (rc_ < 0) { std::fprintf(stderr, "budget_main: %s -> %d (%s)\n", #call, rc_, rtw_last_error()); return 2; } } while (0)
#define EXPECT(call, want) do { const int rc_ = (call); if (rc_ != (want)) { std::fprintf(stderr, "budget_main: %s -> %d, expected %d\n", #call, rc_, (int)(want)); return 3; } } while (0)

static const int W = 40, H = 21, FIRST = 3, N = 5, DEPTH = 4;

template <typename T>
static bool read_file(const std::string& path, std::vector<T>& out, size_t want = 0)
{
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long sz = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    out.resize(sz > 0 ? (size_t)sz / sizeof(T) : 0);
    const size_t n = out.empty() ? 0 : std::fread(out.data(), sizeof(T), out.size(), f);
    std::fclose(f);
    return n == out.size() && !out.empty() && (want == 0 || out.size() == want);
}

static int dump(const std::string& path, const void* data, size_t bytes)
{
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) { std::fprintf(stderr, "budget_main: cannot write %s\n", path.c_str()); return 2; }
    const size_t n = std::fwrite(data, 1, bytes, f);
    std::fclose(f);
    return n == bytes ? 0 : 2;
}

static int build_scene(rtw_context* ctx, const std::string& assets, const std::string& scene_file, rtw_scene** out)
{
    FILE* f = std::fopen(scene_file.c_str(), "r");
    if (!f) { std::fprintf(stderr, "budget_main: cannot read %s\n", scene_file.c_str()); return 2; }
    rtw_scene* scene = nullptr;
    CHECK(rtw_scene_create(ctx, &scene));
    char kind[16], name[64], nodes_file[1024];
    while (std::fscanf(f, "%15s", kind) == 1) {
        float v[7]; int shape = -1, got = 0;
        const std::string k = kind;
        const int nv = k == "sphere" ? 4 : (k == "plane" ? 6 : (k == "capsule" ? 7 : 0));
        for (int i = 0; i < nv; i++) got += std::fscanf(f, "%f", &v[i]);
        if (k == "mesh") got += std::fscanf(f, "%63s", name) - 1;
        if (got != nv || std::fscanf(f, "%1023s", nodes_file) != 1) { std::fprintf(stderr, "budget_main: bad scene line in %s\n", scene_file.c_str()); return 2; }
        if (k == "sphere") CHECK(rtw_scene_add_sphere(scene, v, v[3], &shape));
        else if (k == "plane") CHECK(rtw_scene_add_plane(scene, v, v + 3, &shape));
        else if (k == "capsule") CHECK(rtw_scene_add_capsule(scene, v, v + 3, v[6], &shape));
        else if (k == "mesh") CHECK(rtw_scene_add_mesh_obj(scene, (assets + "/" + name + ".obj").c_str(), &shape));
        else { std::fprintf(stderr, "budget_main: unknown shape %s\n", kind); return 2; }
        std::vector<rtw_material_node> nodes;
        if (!read_file(nodes_file, nodes)) { std::fprintf(stderr, "budget_main: bad node file %s\n", nodes_file); return 2; }
        CHECK(rtw_scene_set_material(scene, shape, nodes.data(), (int)nodes.size()));
    }
    std::fclose(f);
    CHECK(rtw_scene_commit(scene));
    *out = scene;
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: budget_main ASSETS_DIR DIR\n"); return 2; }
    const std::string assets = argv[1], dir = argv[2];
    const size_t npix = (size_t)W * H;
    std::vector<int32_t> budget;
    if (!read_file(dir + "/budget.i32", budget, npix)) { std::fprintf(stderr, "budget_main: bad budget file\n"); return 2; }
    FILE* jobs = std::fopen((dir + "/jobs.txt").c_str(), "r");
    if (!jobs) { std::fprintf(stderr, "budget_main: cannot read the job list\n"); return 2; }
    rtw_context* ctx = nullptr;
    CHECK(rtw_context_create(0, &ctx));
    CHECK(rtw_context_set_option(ctx, "pipeline", 4));
    std::vector<float> accum(npix * 4), start_accum;
    std::vector<uint32_t> argb(npix), start_argb;
    rtw_framebuffer* fb = nullptr;
    CHECK(rtw_framebuffer_wrap(ctx, W, H, accum.data(), argb.data(), &fb));
    char name[96], scene_file[1024];
    int ns, group_max, split_paths, split_min, done = 0;
    while (std::fscanf(jobs, "%95s %1023s %d %d %d %d", name, scene_file, &ns, &group_max, &split_paths, &split_min) == 6) {
        rtw_scene* scene = nullptr;
        const int rc = build_scene(ctx, assets, scene_file, &scene);
        if (rc != 0) return rc;
        CHECK(rtw_framebuffer_clear(fb));
        CHECK(rtw_render_passes(scene, fb, 10, 0, 1, DEPTH, 0, 1, 2, ns, 12345u));
        CHECK(rtw_context_synchronize(ctx));
        start_accum = accum; start_argb = argb;
        for (int k = 0; k <= N + 1; k++) {          // k = 0..N: the uniform snapshots; N + 1: the budgeted call, with the job's grouping
            accum = start_accum; argb = start_argb;
            if (k <= N) CHECK(rtw_render_passes(scene, fb, 10, 0, 1, DEPTH, 0, FIRST, k, ns, 12345u));
            else {
                EXPECT(rtw_render_passes_budget(scene, fb, nullptr, 10, 0, 1, DEPTH, FIRST, N, ns, 12345u), RTW_ERR_INVALID);
                CHECK(rtw_context_set_option(ctx, "group_max", group_max));
                CHECK(rtw_context_set_option(ctx, "split_paths", split_paths));
                CHECK(rtw_context_set_option(ctx, "split_min", split_min));
                CHECK(rtw_render_passes_budget(scene, fb, budget.data(), 10, 0, 1, DEPTH, FIRST, N, ns, 12345u));
                EXPECT(rtw_last_pass_pipeline(ctx), 4);
                CHECK(rtw_context_set_option(ctx, "group_max", 256));
                CHECK(rtw_context_set_option(ctx, "split_paths", 400000));
                CHECK(rtw_context_set_option(ctx, "split_min", 8));
            }
            CHECK(rtw_context_synchronize(ctx));
            const std::string base = dir + "/" + name + (k <= N ? "_k" + std::to_string(k) : std::string());
            if (dump(base + ".accum", accum.data(), accum.size() * 4) || dump(base + ".argb", argb.data(), argb.size() * 4)) return 2;
        }
        CHECK(rtw_scene_destroy(scene));
        done++;
    }
    std::fclose(jobs);
    // rtw_sample_budget at radius 2 over the test's own counts and moments
    std::vector<float> mu;
    if (!read_file(dir + "/sb_accum.f32", accum, npix * 4) || !read_file(dir + "/sb_mu.f32", mu, npix * 2)) { std::fprintf(stderr, "budget_main: bad sample-budget inputs\n"); return 2; }
    CHECK(rtw_framebuffer_destroy(fb));
    CHECK(rtw_framebuffer_wrap(ctx, W, H, accum.data(), argb.data(), &fb));
    rtw_moments* m = nullptr;
    CHECK(rtw_moments_wrap(ctx, W, H, mu.data(), &m));
    rtw_sample_budget_params p;
    CHECK(rtw_sample_budget_default_params(&p));
    p.tolerance = 0.25f; p.min_passes = 2; p.radius = 2;
    std::vector<int32_t> out(npix, -7);
    CHECK(rtw_sample_budget(fb, m, &p, out.data()));
    CHECK(rtw_context_synchronize(ctx));
    if (dump(dir + "/sb.i32", out.data(), out.size() * 4)) return 2;
    p.radius = 3;
    EXPECT(rtw_sample_budget(fb, m, &p, out.data()), RTW_ERR_INVALID);
    CHECK(rtw_moments_destroy(m));
    CHECK(rtw_framebuffer_destroy(fb));
    CHECK(rtw_context_destroy(ctx));
    std::printf("budget_main ok: %d jobs\n", done);
    return 0;
}
