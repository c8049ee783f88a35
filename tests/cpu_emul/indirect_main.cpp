// TEST INFRASTRUCTURE: a stand-alone program over the C ABI of include/rtwin.h on this directory's host build (the HIP stand-in of shim/, ASan + UBSan), run
// directly -- nothing is preloaded.  Per scene of tests/test_indirect_emul.py (24 x 13, pose "offaxis"): the features, then rtw_render_indirect -- two lights,
// 2 gather rays, 2 passes in one call -- under both deals with staging blocks and without them; the frames must be equal word for word.  For the model it
// writes OUT_DIR/SCENE.bin (geom, albedo, ids, camera, accum, argb in a row).  Scenes: camera_support's TORUS and MIXED less its Combine sphere.  usage: indirect_main ASSETS_DIR OUT_DIR
#include <cstdio>
#include <string>
#include <vector>

#include "rtwin.h"

#define CHECK(call) do { const int rc_ = (call); if (rc_ < 0) { std::fprintf(stderr, "indirect_main: %s -> %d (%s)\n", #call, rc_, rtw_last_error()); return 2; } } while (0)

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    const std::string assets = argv[1], outdir = argv[2];
    const int W = 24, H = 13, N = W * H;
    rtw_context* ctx = nullptr;
    CHECK(rtw_context_create(0, &ctx));
    rtw_indirect_params p;
    CHECK(rtw_indirect_default_params(&p));
    p.samples = 2;
    const rtw_light lights[2] = { { RTW_LIGHT_POINT, RTW_LIGHT_INVERSE_SQUARE, { -3.0f, 3.0f, 2.0f }, { 8.0f, 6.0f, 4.0f }, 0.5f },
                                  { RTW_LIGHT_DIRECTIONAL, 0u, { 0.0f, 0.8f, 0.6f }, { 0.5f, 0.6f, 0.7f }, 0.0f } };
    const float up[3] = { 0.0f, 1.0f, 0.0f }, floor_at[3] = { 0.0f, -1.2f, 0.0f }, c1[3] = { 1.9f, 0.2f, -0.5f }, eye[3] = { 4.0f, 2.5f, 5.0f }, target[3] = { 0.1f, -0.1f, 0.0f };
    const rtw_material_node mats[4] = { { RTW_MAT_DIFFUSE_CHECKER, 0.9f, 0.9f, 0.9f, 2.0f, 0, 0, 0 }, { RTW_MAT_REFLECTIVE, 0.9f, 0.9f, 0.9f, 0.0f, 0, 0, 0 },
                                        { RTW_MAT_DIFFUSE, 0.9f, 0.8f, 0.7f, 0.0f, 0, 0, 0 }, { RTW_MAT_DIFFUSE, 1.0f, 1.0f, 1.0f, 0.0f, 0, 0, 0 } };
    for (const std::string which : { "torus", "mixed" }) {
        rtw_scene* scene = nullptr; rtw_features* f = nullptr; rtw_framebuffer* fb = nullptr;
        int idx[3] = { -1, -1, -1 };
        CHECK(rtw_scene_create(ctx, &scene));
        if (which == "mixed") {
            CHECK(rtw_scene_add_plane(scene, up, floor_at, &idx[0]));
            CHECK(rtw_scene_add_sphere(scene, c1, 0.8f, &idx[1]));
        }
        CHECK(rtw_scene_add_mesh_obj(scene, (assets + (which == "mixed" ? "/BlenderMonkey.obj" : "/TorusKnot.obj")).c_str(), &idx[2]));
        for (int k = 0; k < 3; k++) if (idx[k] >= 0) CHECK(rtw_scene_set_material(scene, idx[k], &mats[which == "mixed" ? k : 3], 1));
        rtw_camera cam;
        CHECK(rtw_camera_look_at(eye, target, up, 40.0f, &cam));
        CHECK(rtw_scene_set_camera(scene, &cam));
        CHECK(rtw_features_create(ctx, W, H, &f));
        CHECK(rtw_framebuffer_create(ctx, W, H, &fb));
        CHECK(rtw_scene_commit(scene));
        CHECK(rtw_render_features(scene, f, 10, 0, 1, 0, 1, 1, 12345u));
        std::vector<float> geom(N * 4), albedo(N * 4);
        std::vector<uint32_t> ids(N * 2), accum[3], argb[3];          // (the ids and the sums as words: the comparison is of bits)
        CHECK(rtw_features_read(f, geom.data(), albedo.data(), reinterpret_cast<int32_t*>(ids.data())));
        for (int v = 0; v < 3; v++) {               // deal 0, deal 1, deal 1 with nothing staged
            accum[v].resize(N * 4); argb[v].resize(N);
            CHECK(rtw_context_set_option(ctx, "indirect_deal", v > 0));
            CHECK(rtw_context_set_option(ctx, "indirect_staging", v == 2 ? 0 : 1));
            CHECK(rtw_framebuffer_clear(fb));
            CHECK(rtw_render_indirect(scene, f, lights, 2, &p, 0, 2, 9u, fb));
            CHECK(rtw_framebuffer_read_float(fb, reinterpret_cast<float*>(accum[v].data())));
            CHECK(rtw_framebuffer_resolve_argb(fb, argb[v].data()));
            if (accum[v] != accum[0] || argb[v] != argb[0]) { std::fprintf(stderr, "indirect_main: variant %d differs on %s\n", v, which.c_str()); return 2; }
        }
        FILE* out = std::fopen((outdir + "/" + which + ".bin").c_str(), "wb");
        const bool ok = out && std::fwrite(geom.data(), 16, N, out) + std::fwrite(albedo.data(), 16, N, out) + std::fwrite(ids.data(), 8, N, out) + std::fwrite(&cam, sizeof cam, 1, out) +
                               std::fwrite(accum[0].data(), 16, N, out) + std::fwrite(argb[0].data(), 4, N, out) == (size_t)(5 * N + 1);
        if (!out || std::fclose(out) != 0 || !ok) { std::fprintf(stderr, "indirect_main: cannot write %s.bin\n", which.c_str()); return 2; }
        CHECK(rtw_framebuffer_destroy(fb));
        CHECK(rtw_features_destroy(f));
        CHECK(rtw_scene_destroy(scene));
    }
    CHECK(rtw_context_destroy(ctx));
    std::printf("indirect_main ok\n");
    return 0;
}
