// TEST INFRASTRUCTURE: a stand-alone program over the C ABI of include/rtwin.h, linked against the objects of this directory's host build
// (the product's own sources on the HIP stand-in of shim/, AddressSanitizer + UBSan) and run directly -- nothing is preloaded.
// It renders TorusKnot under material trees read from files through the pipelines 0, 3 and 4 and dumps accumulator and ARGB words as raw
// files; tests/test_material_emul.py writes the job list and the node arrays and compares the dumps with the oracle.
//
// usage: material_main ASSETS_DIR OUT_DIR JOBS_FILE
// a job line:  name nodes_file pipeline width height sub_samples depth preview n_passes bad_nodes_file
//   nodes_file: rtw_material_node records (32 bytes each).  bad_nodes_file: "-", or a file of trees the library must refuse -- per tree an
//   int32 count, an int32 expected return code and count (at least one) node records; each is offered to rtw_scene_set_material after the
//   good tree was set, and the frame must then still be the good tree's.  With a bad_nodes_file the job also asks for max_bounce 17.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rtwin.h"

#define CHECK(call) do { const int rc_ = (call); if (rc_ < 0) { std::fprintf(stderr, "material_main: %s -> %d (%s)\n", #call, rc_, rtw_last_error()); return 2; } } while (0)
#define EXPECT(call, want) do { const int rc_ = (call); if (rc_ != (want)) { std::fprintf(stderr, "material_main: %s -> %d, expected %d\n", #call, rc_, (int)(want)); return 3; } } while (0)

static bool slurp(const std::string& path, std::vector<unsigned char>& out)
{
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long sz = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    out.resize(sz > 0 ? (size_t)sz : 0);
    const size_t n = out.empty() ? 0 : std::fread(out.data(), 1, out.size(), f);
    std::fclose(f);
    return n == out.size();
}

static int dump(const std::string& path, const void* data, size_t bytes)
{
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) { std::fprintf(stderr, "material_main: cannot write %s\n", path.c_str()); return 2; }
    const size_t n = std::fwrite(data, 1, bytes, f);
    std::fclose(f);
    return n == bytes ? 0 : 2;
}

// every tree of the file is refused with its stated code
static int offer_bad_trees(rtw_scene* scene, int shape, const std::string& path, int* offered)
{
    std::vector<unsigned char> raw;
    if (!slurp(path, raw)) { std::fprintf(stderr, "material_main: cannot read %s\n", path.c_str()); return 2; }
    size_t at = 0;
    while (at + 8 <= raw.size()) {
        int32_t head[2];
        std::memcpy(head, raw.data() + at, 8);
        at += 8;
        const size_t held = (size_t)(head[0] > 0 ? head[0] : 1);
        if (at + held * sizeof(rtw_material_node) > raw.size()) { std::fprintf(stderr, "material_main: %s is cut short\n", path.c_str()); return 2; }
        std::vector<rtw_material_node> nodes(held);
        std::memcpy(nodes.data(), raw.data() + at, held * sizeof(rtw_material_node));
        at += held * sizeof(rtw_material_node);
        EXPECT(rtw_scene_set_material(scene, shape, nodes.data(), head[0]), head[1]);
        (*offered)++;
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 4) { std::fprintf(stderr, "usage: material_main ASSETS_DIR OUT_DIR JOBS_FILE\n"); return 2; }
    const std::string assets = argv[1], outdir = argv[2];
    FILE* jobs = std::fopen(argv[3], "r");
    if (!jobs) { std::fprintf(stderr, "material_main: cannot read %s\n", argv[3]); return 2; }
    FILE* report = std::fopen((outdir + "/report.txt").c_str(), "w");
    if (!report) { std::fprintf(stderr, "material_main: cannot write the report\n"); return 2; }
    rtw_context* ctx = nullptr;
    CHECK(rtw_context_create(0, &ctx));
    char name[96], nodes_file[1024], bad_file[1024];
    int pipeline, W, H, ns, depth, preview, n_passes, done = 0;
    while (std::fscanf(jobs, "%95s %1023s %d %d %d %d %d %d %d %1023s", name, nodes_file, &pipeline, &W, &H, &ns, &depth, &preview, &n_passes, bad_file) == 10) {
        std::vector<unsigned char> raw;
        if (!slurp(nodes_file, raw) || raw.empty() || raw.size() % sizeof(rtw_material_node)) { std::fprintf(stderr, "material_main: bad node file %s\n", nodes_file); return 2; }
        std::vector<rtw_material_node> nodes(raw.size() / sizeof(rtw_material_node));
        std::memcpy(nodes.data(), raw.data(), raw.size());
        CHECK(rtw_context_set_option(ctx, "pipeline", pipeline));
        rtw_scene* scene = nullptr;
        CHECK(rtw_scene_create(ctx, &scene));
        int shape = -1, offered = 0;
        CHECK(rtw_scene_add_mesh_obj(scene, (assets + "/TorusKnot.obj").c_str(), &shape));
        CHECK(rtw_scene_set_material(scene, shape, nodes.data(), (int)nodes.size()));
        const bool with_bad = std::string(bad_file) != "-";
        if (with_bad && offer_bad_trees(scene, shape, bad_file, &offered) != 0) return 3;
        CHECK(rtw_scene_commit(scene));
        rtw_framebuffer* fb = nullptr;
        CHECK(rtw_framebuffer_create(ctx, W, H, &fb));
        CHECK(rtw_framebuffer_clear(fb));
        if (with_bad) {      // the bounce limit: 17 is refused by both entries, and nothing was rendered
            const float ray[7] = { 0.0f, 0.0f, 7.0f, 0.0f, 0.0f, -1.0f, 1000.0f };
            const uint32_t key[2] = { 0u, 0u };
            float rgb[3];
            EXPECT(rtw_render_passes(scene, fb, 10, 0, 1, RTW_MAX_BOUNCE + 1, 0, 0, 1, ns, 20261021u), RTW_ERR_LIMIT);
            EXPECT(rtw_ray_trace(scene, ray, key, 1, RTW_MAX_BOUNCE + 1, 0, 20261021u, W, H, rgb), RTW_ERR_LIMIT);
            CHECK(rtw_ray_trace(scene, ray, key, 1, RTW_MAX_BOUNCE, 0, 20261021u, W, H, rgb));
        }
        CHECK(rtw_render_passes(scene, fb, 10, 0, 1, depth, preview, 0, n_passes, ns, 20261021u));
        const int ran = rtw_last_pass_pipeline(ctx);
        std::vector<float> accum((size_t)W * H * 4);
        std::vector<uint32_t> argb((size_t)W * H);
        CHECK(rtw_framebuffer_read_float(fb, accum.data()));
        CHECK(rtw_framebuffer_resolve_argb(fb, argb.data()));
        if (dump(outdir + "/" + name + ".accum", accum.data(), accum.size() * 4) || dump(outdir + "/" + name + ".argb", argb.data(), argb.size() * 4)) return 2;
        std::fprintf(report, "%s %d %d\n", name, ran, offered);
        CHECK(rtw_framebuffer_destroy(fb));
        CHECK(rtw_scene_destroy(scene));
        done++;
    }
    std::fclose(jobs);
    std::fclose(report);
    CHECK(rtw_context_destroy(ctx));
    std::printf("material_main ok: %d frames\n", done);
    return 0;
}
