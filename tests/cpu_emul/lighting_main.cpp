// TEST INFRASTRUCTURE: a stand-alone program over the C ABI of include/rtwin.h, linked against the objects of this directory's host build
// (the product's own sources on the HIP stand-in of shim/, AddressSanitizer + UBSan) and run directly -- nothing is preloaded.
// It renders the features of one 24 x 13 frame of TorusKnot and one of the multi-shape scene (tests/camera_support.py TORUS / MIXED, pose "offaxis"),
// then rtw_render_lighting -- two lights (tests/test_lighting_emul.py LIGHTS), 3 samples, 2 passes in one call -- under both "lighting_deal" values, and
// dumps the features and the framebuffers as raw files; tests/test_lighting_emul.py compares them with the model of tests/lighting_support.py.
//
// usage: lighting_main ASSETS_DIR OUT_DIR
// dumps SCENE.geom / .albedo / .ids / .cam and SCENE_dK.accum / .argb
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "rtwin.h"

#define CHECK(call) do { const int rc_ = (call); if (rc_ < 0) { std::fprintf(stderr, "lighting_main: %s -> %d (%s)\n", #call, rc_, rtw_last_error()); return 2; } } while (0)

static int build_scene(rtw_context* ctx, const std::string& which, const std::string& assets, rtw_scene** out)
{
    rtw_scene* s = nullptr;
    CHECK(rtw_scene_create(ctx, &s));
    int idx = -1;
    if (which == "torus") {
        CHECK(rtw_scene_add_mesh_obj(s, (assets + "/TorusKnot.obj").c_str(), &idx));
    } else {            // the geometry of MIXED; the albedo is read from the dumped features
        const float n[3] = { 0.0f, 1.0f, 0.0f }, p[3] = { 0.0f, -1.2f, 0.0f }, c1[3] = { 1.9f, 0.2f, -0.5f }, c2[3] = { -1.9f, -0.3f, 0.6f };
        CHECK(rtw_scene_add_plane(s, n, p, &idx));
        CHECK(rtw_scene_add_sphere(s, c1, 0.8f, &idx));
        CHECK(rtw_scene_add_sphere(s, c2, 0.6f, &idx));
        CHECK(rtw_scene_add_mesh_obj(s, (assets + "/BlenderMonkey.obj").c_str(), &idx));
    }
    const float e[3] = { 4.0f, 2.5f, 5.0f }, t[3] = { 0.1f, -0.1f, 0.0f }, u[3] = { 0.0f, 1.0f, 0.0f };
    rtw_camera cam;
    CHECK(rtw_camera_look_at(e, t, u, 40.0f, &cam));
    CHECK(rtw_scene_set_camera(s, &cam));
    *out = s;
    return 0;
}

static int dump(const std::string& path, const void* data, size_t bytes)
{
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) { std::fprintf(stderr, "lighting_main: cannot write %s\n", path.c_str()); return 2; }
    const size_t n = std::fwrite(data, 1, bytes, f);
    std::fclose(f);
    return n == bytes ? 0 : 2;
}

int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: lighting_main ASSETS_DIR OUT_DIR\n"); return 2; }
    const std::string assets = argv[1], outdir = argv[2];
    const int W = 24, H = 13;
    rtw_context* ctx = nullptr;
    CHECK(rtw_context_create(0, &ctx));
    rtw_lighting_params p;
    CHECK(rtw_lighting_default_params(&p));
    p.samples = 3;
    const rtw_light lights[2] = { { RTW_LIGHT_POINT, RTW_LIGHT_INVERSE_SQUARE, { -3.0f, 3.0f, 2.0f }, { 8.0f, 6.0f, 4.0f }, 0.5f },
                                  { RTW_LIGHT_DIRECTIONAL, 0u, { 0.0f, 0.8f, 0.6f }, { 0.5f, 0.6f, 0.7f }, 0.0f } };
    int done = 0;
    for (const char* which : { "torus", "mixed" }) {
        rtw_scene* scene = nullptr;
        if (build_scene(ctx, which, assets, &scene) != 0) return 2;
        rtw_features* f = nullptr; rtw_framebuffer* fb = nullptr;
        CHECK(rtw_features_create(ctx, W, H, &f));
        CHECK(rtw_framebuffer_create(ctx, W, H, &fb));
        if (rtw_render_lighting(scene, f, lights, 2, &p, 0, 2, 9u, fb) != RTW_ERR_STATE) { std::fprintf(stderr, "lighting_main: an uncommitted scene was accepted\n"); return 2; }
        CHECK(rtw_scene_commit(scene));
        CHECK(rtw_render_features(scene, f, 10, 0, 1, 0, 1, 1, 12345u));
        std::vector<float> geom((size_t)W * H * 4), albedo((size_t)W * H * 4), accum((size_t)W * H * 4);
        std::vector<int32_t> ids((size_t)W * H * 2);
        std::vector<uint32_t> argb((size_t)W * H);
        CHECK(rtw_features_read(f, geom.data(), albedo.data(), ids.data()));
        rtw_camera cam;
        CHECK(rtw_scene_get_camera(scene, &cam));
        const std::string base = outdir + "/" + which;
        if (dump(base + ".geom", geom.data(), geom.size() * 4) || dump(base + ".albedo", albedo.data(), albedo.size() * 4) ||
            dump(base + ".ids", ids.data(), ids.size() * 4) || dump(base + ".cam", &cam, sizeof cam)) return 2;
        for (int deal = 0; deal < 2; deal++) {
            CHECK(rtw_context_set_option(ctx, "lighting_deal", deal));
            CHECK(rtw_framebuffer_clear(fb));
            CHECK(rtw_render_lighting(scene, f, lights, 2, &p, 0, 2, 9u, fb));
            CHECK(rtw_framebuffer_read_float(fb, accum.data()));
            CHECK(rtw_framebuffer_resolve_argb(fb, argb.data()));
            const std::string o = base + "_d" + std::to_string(deal);
            if (dump(o + ".accum", accum.data(), accum.size() * 4) || dump(o + ".argb", argb.data(), argb.size() * 4)) return 2;
            done++;
        }
        CHECK(rtw_framebuffer_destroy(fb));
        CHECK(rtw_features_destroy(f));
        CHECK(rtw_scene_destroy(scene));
    }
    CHECK(rtw_context_destroy(ctx));
    std::printf("lighting_main ok: %d frames\n", done);
    return 0;
}
