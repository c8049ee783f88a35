// TEST INFRASTRUCTURE: a stand-alone program over the C ABI of include/rtwin.h, linked against the objects of this directory's host build
// (the product's own sources on the HIP stand-in of shim/, AddressSanitizer + UBSan) and run directly -- nothing is preloaded.
// It renders frames through a thin lens with the pipelines 4 (both lens routes), 3 and 0 and dumps accumulator and ARGB words as raw files;
// tests/test_lens_emul.py writes the job list and compares the dumps with the oracle.
//
// usage: lens_main ASSETS_DIR OUT_DIR JOBS_FILE
// a job line:  name scene ex ey ez tx ty tz ux uy uz vfov radius focus pipeline lens_route width height n_passes sub_samples depth begin end
//   scene = torus | mixed (tests/camera_support.py TORUS / MIXED); radius < 0: no lens is ever set; begin < 0: the whole frame
//   (rtw_render_passes), else the pixels begin .. end pass by pass (rtw_render_range)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "rtwin.h"

#define CHECK(call) do { const int rc_ = (call); if (rc_ < 0) { std::fprintf(stderr, "lens_main: %s -> %d (%s)\n", #call, rc_, rtw_last_error()); return 2; } } while (0)

static rtw_material_node leaf(int type, float r, float g, float b, float param) { const rtw_material_node n = { type, r, g, b, param, 0, 0, 0 }; return n; }

static int build_scene(rtw_context* ctx, const std::string& which, const std::string& assets, rtw_scene** out, int* mesh_shape)
{
    rtw_scene* s = nullptr;
    CHECK(rtw_scene_create(ctx, &s));
    int idx = -1;
    if (which == "torus") {
        CHECK(rtw_scene_add_mesh_obj(s, (assets + "/TorusKnot.obj").c_str(), &idx));
        const rtw_material_node m = leaf(RTW_MAT_DIFFUSE, 1.0f, 1.0f, 1.0f, 0.0f);
        CHECK(rtw_scene_set_material(s, idx, &m, 1));
        *mesh_shape = idx;
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
        *mesh_shape = idx;
    } else {
        std::fprintf(stderr, "lens_main: unknown scene %s\n", which.c_str());
        return 2;
    }
    *out = s;
    return 0;
}

static int dump(const std::string& path, const void* data, size_t bytes)
{
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) { std::fprintf(stderr, "lens_main: cannot write %s\n", path.c_str()); return 2; }
    const size_t n = std::fwrite(data, 1, bytes, f);
    std::fclose(f);
    return n == bytes ? 0 : 2;
}

int main(int argc, char** argv)
{
    if (argc != 4) { std::fprintf(stderr, "usage: lens_main ASSETS_DIR OUT_DIR JOBS_FILE\n"); return 2; }
    const std::string assets = argv[1], outdir = argv[2];
    FILE* jobs = std::fopen(argv[3], "r");
    if (!jobs) { std::fprintf(stderr, "lens_main: cannot read %s\n", argv[3]); return 2; }
    FILE* report = std::fopen((outdir + "/report.txt").c_str(), "w");
    if (!report) { std::fprintf(stderr, "lens_main: cannot write the report\n"); return 2; }
    rtw_context* ctx = nullptr;
    CHECK(rtw_context_create(0, &ctx));
    char name[96], scene_name[32];
    float e[3], t[3], u[3], vfov, radius, focus;
    int pipeline, route, W, H, n_passes, ns, depth, begin, end, done = 0;
    while (std::fscanf(jobs, "%95s %31s %f %f %f %f %f %f %f %f %f %f %f %f %d %d %d %d %d %d %d %d %d", name, scene_name, &e[0], &e[1], &e[2], &t[0], &t[1], &t[2],
                       &u[0], &u[1], &u[2], &vfov, &radius, &focus, &pipeline, &route, &W, &H, &n_passes, &ns, &depth, &begin, &end) == 23) {
        CHECK(rtw_context_set_option(ctx, "pipeline", pipeline));
        CHECK(rtw_context_set_option(ctx, "lens_route", route));
        rtw_scene* scene = nullptr; int mesh_shape = -1;
        if (build_scene(ctx, scene_name, assets, &scene, &mesh_shape) != 0) return 2;
        rtw_camera cam;
        CHECK(rtw_camera_look_at(e, t, u, vfov, &cam));
        CHECK(rtw_scene_set_camera(scene, &cam));
        CHECK(rtw_scene_commit(scene));
        if (radius >= 0.0f) {       // after commit: the path that drops the cached tables
            const rtw_lens lens = { radius, focus };
            CHECK(rtw_scene_set_lens(scene, &lens));
        }
        rtw_framebuffer* fb = nullptr;
        CHECK(rtw_framebuffer_create(ctx, W, H, &fb));
        CHECK(rtw_framebuffer_clear(fb));
        if (begin < 0) CHECK(rtw_render_passes(scene, fb, 10, 0, 1, depth, 0, 0, n_passes, ns, 12345u));
        else for (int p = 0; p < n_passes; p++) CHECK(rtw_render_range(scene, fb, begin, end, depth, 0, p, ns, 12345u));
        const int ran = rtw_last_pass_pipeline(ctx);
        std::vector<float> accum((size_t)W * H * 4);
        std::vector<uint32_t> argb((size_t)W * H);
        CHECK(rtw_framebuffer_read_float(fb, accum.data()));
        CHECK(rtw_framebuffer_resolve_argb(fb, argb.data()));
        int64_t counts[2] = { 0, 0 };
        const int has_bins = rtw_scene_mesh_bins(scene, mesh_shape, W, H, 16, 4, nullptr, 0, nullptr, 0, counts);
        CHECK(has_bins);
        rtw_lens back = { -1.0f, -1.0f };
        CHECK(rtw_scene_get_lens(scene, &back));
        if (dump(outdir + "/" + name + ".accum", accum.data(), accum.size() * 4) || dump(outdir + "/" + name + ".argb", argb.data(), argb.size() * 4) ||
            dump(outdir + "/" + name + ".lens", &back, sizeof back)) return 2;
        std::fprintf(report, "%s %d %d\n", name, ran, has_bins);
        CHECK(rtw_framebuffer_destroy(fb));
        CHECK(rtw_scene_destroy(scene));
        done++;
    }
    std::fclose(jobs);
    std::fclose(report);
    CHECK(rtw_context_destroy(ctx));
    std::printf("lens_main ok: %d frames\n", done);
    return 0;
}
