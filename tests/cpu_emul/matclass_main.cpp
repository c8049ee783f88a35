// TEST INFRASTRUCTURE: a stand-alone program over the C ABI of include/rtwin.h, linked against the objects of this directory's host build
// (the product's own sources on the HIP stand-in of shim/, AddressSanitizer + UBSan) and run directly -- nothing is preloaded.
// It renders one-mesh scenes under material trees read from files through pipeline 4 with option "material_variants" as the job says, dumps
// accumulator and ARGB words as raw files and reports the material class each call's shade / primary kernels were instantiated for;
// tests/test_matclass_emul.py writes the job list and the node arrays and compares the dumps with the oracle.
//
// usage: matclass_main ASSETS_DIR OUT_DIR JOBS_FILE
// a job line:  name mesh nodes_file nodes_file2 variants split_paths primary_passes cam ex ey ez tx ty tz ux uy uz vfov width height n_passes sub_samples depth
//   nodes_file: rtw_material_node records (32 bytes each), or "-": the mesh gets no material.  cam 0: no camera is ever set (the numbers are read and dropped).
//   nodes_file2 other than "-": the class follows the commit -- after the first frame (dumped as NAME) a committed scene must refuse another material,
//   then a scene of the same mesh is committed under the second tree in the same context and rendered into the same, cleared framebuffer (dumped as NAME_re).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rtwin.h"

#define CHECK(call) do { const int rc_ = (call); if (rc_ < 0) { std::fprintf(stderr, "matclass_main: %s -> %d (%s)\n", #call, rc_, rtw_last_error()); return 2; } } while (0)
#define EXPECT(call, want) do { const int rc_ = (call); if (rc_ != (want)) { std::fprintf(stderr, "matclass_main: %s -> %d, expected %d\n", #call, rc_, (int)(want)); return 3; } } while (0)

static bool read_nodes(const std::string& path, std::vector<rtw_material_node>& out)
{
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long sz = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    if (sz <= 0 || (size_t)sz % sizeof(rtw_material_node)) { std::fclose(f); return false; }
    out.resize((size_t)sz / sizeof(rtw_material_node));
    const size_t n = std::fread(out.data(), sizeof(rtw_material_node), out.size(), f);
    std::fclose(f);
    return n == out.size();
}

static int dump(const std::string& path, const void* data, size_t bytes)
{
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) { std::fprintf(stderr, "matclass_main: cannot write %s\n", path.c_str()); return 2; }
    const size_t n = std::fwrite(data, 1, bytes, f);
    std::fclose(f);
    return n == bytes ? 0 : 2;
}

struct Job { int cam; float e[3], t[3], u[3], vfov; int W, H, n_passes, ns, depth; };

// one scene of `mesh` under the tree of `nodes_file`, committed, rendered into fb (cleared first) and dumped as `name`; a line of the report
static int frame(rtw_context* ctx, rtw_framebuffer* fb, const std::string& assets, const std::string& outdir, const std::string& name, const std::string& mesh,
                 const std::string& nodes_file, const Job& j, bool offer_after_commit, FILE* report)
{
    rtw_scene* scene = nullptr;
    CHECK(rtw_scene_create(ctx, &scene));
    int shape = -1;
    CHECK(rtw_scene_add_mesh_obj(scene, (assets + "/" + mesh + ".obj").c_str(), &shape));
    std::vector<rtw_material_node> nodes;
    if (nodes_file != "-") {
        if (!read_nodes(nodes_file, nodes)) { std::fprintf(stderr, "matclass_main: bad node file %s\n", nodes_file.c_str()); return 2; }
        CHECK(rtw_scene_set_material(scene, shape, nodes.data(), (int)nodes.size()));
    }
    if (j.cam) {
        rtw_camera cam;
        CHECK(rtw_camera_look_at(j.e, j.t, j.u, j.vfov, &cam));
        CHECK(rtw_scene_set_camera(scene, &cam));
    }
    CHECK(rtw_scene_commit(scene));
    CHECK(rtw_framebuffer_clear(fb));
    CHECK(rtw_render_passes(scene, fb, 10, 0, 1, j.depth, 0, 0, j.n_passes, j.ns, 12345u));
    const int ran = rtw_last_pass_pipeline(ctx), cls = rtw_last_pass_material_class(ctx);
    if (offer_after_commit) {       // a scene's trees are final once it is committed: its class cannot go stale
        EXPECT(rtw_scene_set_material(scene, shape, nodes.data(), (int)nodes.size()), RTW_ERR_STATE);
        EXPECT(rtw_scene_commit(scene), RTW_ERR_STATE);
    }
    std::vector<float> accum((size_t)j.W * j.H * 4);
    std::vector<uint32_t> argb((size_t)j.W * j.H);
    CHECK(rtw_framebuffer_read_float(fb, accum.data()));
    CHECK(rtw_framebuffer_resolve_argb(fb, argb.data()));
    if (dump(outdir + "/" + name + ".accum", accum.data(), accum.size() * 4) || dump(outdir + "/" + name + ".argb", argb.data(), argb.size() * 4)) return 2;
    std::fprintf(report, "%s %d %d\n", name.c_str(), ran, cls);
    CHECK(rtw_scene_destroy(scene));
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 4) { std::fprintf(stderr, "usage: matclass_main ASSETS_DIR OUT_DIR JOBS_FILE\n"); return 2; }
    const std::string assets = argv[1], outdir = argv[2];
    FILE* jobs = std::fopen(argv[3], "r");
    if (!jobs) { std::fprintf(stderr, "matclass_main: cannot read %s\n", argv[3]); return 2; }
    FILE* report = std::fopen((outdir + "/report.txt").c_str(), "w");
    if (!report) { std::fprintf(stderr, "matclass_main: cannot write the report\n"); return 2; }
    rtw_context* ctx = nullptr;
    CHECK(rtw_context_create(0, &ctx));
    EXPECT(rtw_last_pass_material_class(ctx), -1);       // nothing rendered yet
    CHECK(rtw_context_set_option(ctx, "pipeline", 4));
    char name[96], mesh[64], nodes_file[1024], nodes_file2[1024];
    int variants, split_paths, primary_passes, done = 0;
    Job j;
    while (std::fscanf(jobs, "%95s %63s %1023s %1023s %d %d %d %d %f %f %f %f %f %f %f %f %f %f %d %d %d %d %d", name, mesh, nodes_file, nodes_file2, &variants, &split_paths,
                       &primary_passes, &j.cam, &j.e[0], &j.e[1], &j.e[2], &j.t[0], &j.t[1], &j.t[2], &j.u[0], &j.u[1], &j.u[2], &j.vfov, &j.W, &j.H, &j.n_passes, &j.ns, &j.depth) == 23) {
        CHECK(rtw_context_set_option(ctx, "material_variants", variants));
        CHECK(rtw_context_set_option(ctx, "split_paths", split_paths));
        CHECK(rtw_context_set_option(ctx, "primary_passes", primary_passes));
        rtw_framebuffer* fb = nullptr;
        CHECK(rtw_framebuffer_create(ctx, j.W, j.H, &fb));
        const bool again = std::string(nodes_file2) != "-";
        int rc = frame(ctx, fb, assets, outdir, name, mesh, nodes_file, j, again, report);
        if (rc != 0) return rc;
        done++;
        if (again) {
            rc = frame(ctx, fb, assets, outdir, std::string(name) + "_re", mesh, nodes_file2, j, false, report);
            if (rc != 0) return rc;
            done++;
        }
        CHECK(rtw_framebuffer_destroy(fb));
    }
    std::fclose(jobs);
    std::fclose(report);
    CHECK(rtw_context_destroy(ctx));
    std::printf("matclass_main ok: %d frames\n", done);
    return 0;
}
