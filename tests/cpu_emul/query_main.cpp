// TEST INFRASTRUCTURE: a stand-alone program over the C ABI of include/rtwin.h, linked against the objects of this directory's host build
// (the product's own sources on the HIP stand-in of shim/, AddressSanitizer + UBSan) and run directly -- nothing is preloaded.
// It runs the device-buffer ray queries (rtw_trace_closest_device / rtw_trace_occluded_device; in the emulation a device pointer is a host
// pointer) and dumps their outputs as raw files; tests/test_query_emul.py writes the scenes, rays and job list and compares the dumps.
//
// usage: query_main ASSETS_DIR OUT_DIR JOBS_FILE
// a job line:  name scene_file rays_file n prune query_kernel query_blocks mode
//   scene_file: one shape per line, in insertion order:  mesh NAME | sphere c3 r | plane n3 p3 | capsule a3 b3 r | triangle a3 b3 c3
//   rays_file: raw float32, 7 per ray; the job takes its first n
//   mode 0: every output; 1: tri NULL; 2: only shape; 3: shape and tri, hits NULL (the triangle's index without the finish)
// dumps name.hits / name.shape / name.tri (the outputs asked for) and name.occ; a report line per job:
//   name  rays boxes tris hits (closest)  rays boxes tris (any-hit)  guards_intact  rtw_trace_occluded (host arrays, mode 2 only) == device bytes
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "rtwin.h"

#define CHECK(call) do { const int rc_ = (call); if (rc_ < 0) { std::fprintf(stderr, "query_main: %s -> %d (%s)\n", #call, rc_, rtw_last_error()); return 2; } } while (0)

static int build_scene(rtw_context* ctx, const std::string& file, const std::string& assets, rtw_scene** out)
{
    FILE* f = std::fopen(file.c_str(), "r");
    if (!f) { std::fprintf(stderr, "query_main: cannot read %s\n", file.c_str()); return 2; }
    rtw_scene* s = nullptr;
    CHECK(rtw_scene_create(ctx, &s));
    char kind[32], name[64];
    int idx = -1;
    while (std::fscanf(f, "%31s", kind) == 1) {
        const std::string k = kind;
        float a[3], b[3], c[3], r;
        if (k == "mesh" && std::fscanf(f, "%63s", name) == 1) CHECK(rtw_scene_add_mesh_obj(s, (assets + "/" + name + ".obj").c_str(), &idx));
        else if (k == "sphere" && std::fscanf(f, "%f %f %f %f", &a[0], &a[1], &a[2], &r) == 4) CHECK(rtw_scene_add_sphere(s, a, r, &idx));
        else if (k == "plane" && std::fscanf(f, "%f %f %f %f %f %f", &a[0], &a[1], &a[2], &b[0], &b[1], &b[2]) == 6) CHECK(rtw_scene_add_plane(s, a, b, &idx));
        else if (k == "capsule" && std::fscanf(f, "%f %f %f %f %f %f %f", &a[0], &a[1], &a[2], &b[0], &b[1], &b[2], &r) == 7) CHECK(rtw_scene_add_capsule(s, a, b, r, &idx));
        else if (k == "triangle" && std::fscanf(f, "%f %f %f %f %f %f %f %f %f", &a[0], &a[1], &a[2], &b[0], &b[1], &b[2], &c[0], &c[1], &c[2]) == 9) CHECK(rtw_scene_add_triangle(s, a, b, c, &idx));
        else { std::fprintf(stderr, "query_main: bad shape line in %s\n", file.c_str()); return 2; }
    }
    std::fclose(f);
    CHECK(rtw_scene_commit(s));
    *out = s;
    return 0;
}

static int dump(const std::string& path, const void* data, size_t bytes)
{
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) { std::fprintf(stderr, "query_main: cannot write %s\n", path.c_str()); return 2; }
    const size_t n = std::fwrite(data, 1, bytes, f);
    std::fclose(f);
    return n == bytes ? 0 : 2;
}

// an output buffer of exactly `bytes` with 64 guard bytes on either side
struct Guarded {
    std::vector<unsigned char> mem; size_t bytes;
    explicit Guarded(size_t b) : mem(b + 128, 0xA5), bytes(b) {}
    void* p() { return mem.data() + 64; }
    bool intact() const { for (size_t i = 0; i < 64; i++) if (mem[i] != 0xA5 || mem[64 + bytes + i] != 0xA5) return false; return true; }
};

int main(int argc, char** argv)
{
    if (argc != 4) { std::fprintf(stderr, "usage: query_main ASSETS_DIR OUT_DIR JOBS_FILE\n"); return 2; }
    const std::string assets = argv[1], outdir = argv[2];
    FILE* jobs = std::fopen(argv[3], "r");
    if (!jobs) { std::fprintf(stderr, "query_main: cannot read %s\n", argv[3]); return 2; }
    FILE* report = std::fopen((outdir + "/report.txt").c_str(), "w");
    if (!report) { std::fprintf(stderr, "query_main: cannot write the report\n"); return 2; }
    rtw_context* ctx = nullptr;
    CHECK(rtw_context_create(0, &ctx));
    CHECK(rtw_stats_enable(ctx, 1));
    // the option names exist only where a context does; an unknown value is refused
    if (rtw_context_set_option(ctx, "query_blocks_", 7) != RTW_ERR_INVALID || rtw_context_set_option(ctx, "query_kernels", 1) != RTW_ERR_INVALID) {
        std::fprintf(stderr, "query_main: a bad option was accepted\n"); return 2;
    }
    std::map<std::string, rtw_scene*> scenes;
    std::map<std::string, std::vector<float>> ray_files;
    char name[96], scene_file[512], rays_file[512];
    long long n; int prune, qk, qb, mode, done = 0;
    while (std::fscanf(jobs, "%95s %511s %511s %lld %d %d %d %d", name, scene_file, rays_file, &n, &prune, &qk, &qb, &mode) == 8) {
        if (!scenes.count(scene_file)) { rtw_scene* s = nullptr; if (build_scene(ctx, scene_file, assets, &s) != 0) return 2; scenes[scene_file] = s; }
        rtw_scene* scene = scenes[scene_file];
        if (!ray_files.count(rays_file)) {
            FILE* rf = std::fopen(rays_file, "rb");
            if (!rf) { std::fprintf(stderr, "query_main: cannot read %s\n", rays_file); return 2; }
            std::vector<float> v; float buf[7 * 256]; size_t got;
            while ((got = std::fread(buf, 4, 7 * 256, rf)) > 0) v.insert(v.end(), buf, buf + got);
            std::fclose(rf);
            ray_files[rays_file] = v;
        }
        const std::vector<float>& all = ray_files[rays_file];
        if (n < 0 || (size_t)n * 7 > all.size()) { std::fprintf(stderr, "query_main: %s asks for more rays than %s holds\n", name, rays_file); return 2; }
        // exactly n rays in a block of their own: a read past n * 7 floats is a heap overflow the sanitizer reports
        std::vector<float> rays(all.begin(), all.begin() + (size_t)n * 7);
        CHECK(rtw_scene_set_prune(scene, prune));
        CHECK(rtw_context_set_option(ctx, "query_kernel", qk));
        CHECK(rtw_context_set_option(ctx, "query_blocks", qb));
        Guarded hits((size_t)n * 44), shape((size_t)n * 4), tri((size_t)n * 4), occ((size_t)n), occ_host((size_t)n);
        rtw_stats sc, sa;
        CHECK(rtw_stats_reset(ctx));
        CHECK(rtw_trace_closest_device(scene, rays.data(), n, mode == 0 || mode == 1 ? hits.p() : nullptr, shape.p(), mode == 0 || mode == 3 ? tri.p() : nullptr));
        CHECK(rtw_context_synchronize(ctx));
        CHECK(rtw_stats_get(ctx, &sc));
        CHECK(rtw_stats_reset(ctx));
        CHECK(rtw_trace_occluded_device(scene, rays.data(), n, occ.p()));
        CHECK(rtw_context_synchronize(ctx));
        CHECK(rtw_stats_get(ctx, &sa));
        if (mode == 2) CHECK(rtw_trace_occluded(scene, rays.data(), n, (uint8_t*)occ_host.p()));       // the host entry: once per scene is enough
        const bool guards = hits.intact() && shape.intact() && tri.intact() && occ.intact() && occ_host.intact();
        const bool host_same = mode != 2 || std::memcmp(occ.p(), occ_host.p(), (size_t)n) == 0;
        const std::string base = outdir + "/" + name;
        if ((mode <= 1 && dump(base + ".hits", hits.p(), hits.bytes)) || dump(base + ".shape", shape.p(), shape.bytes) ||
            ((mode == 0 || mode == 3) && dump(base + ".tri", tri.p(), tri.bytes)) || dump(base + ".occ", occ.p(), occ.bytes)) return 2;
        std::fprintf(report, "%s %llu %llu %llu %llu %llu %llu %llu %d %d\n", name, (unsigned long long)sc.rays, (unsigned long long)sc.box_tests, (unsigned long long)sc.tri_tests,
                     (unsigned long long)sc.shaded_hits, (unsigned long long)sa.rays, (unsigned long long)sa.box_tests, (unsigned long long)sa.tri_tests, guards ? 1 : 0, host_same ? 1 : 0);
        done++;
    }
    std::fclose(jobs);
    std::fclose(report);
    // argument errors of the new entry points (a context exists here, unlike in the CPU suite)
    {
        rtw_scene* fresh = nullptr; float r[7] = { 0, 0, 0, 0, 0, 1, 1 }; uint8_t o = 0; int32_t sh = 0;
        CHECK(rtw_scene_create(ctx, &fresh));
        const bool ok = rtw_trace_closest_device(fresh, r, 1, nullptr, &sh, nullptr) == RTW_ERR_STATE && rtw_trace_occluded_device(fresh, r, 1, &o) == RTW_ERR_STATE &&
                        rtw_trace_occluded(fresh, r, 1, &o) == RTW_ERR_STATE;
        CHECK(rtw_scene_destroy(fresh));
        bool ok2 = true;
        if (!scenes.empty()) {
            rtw_scene* s = scenes.begin()->second;
            ok2 = rtw_trace_closest_device(s, r, 1, nullptr, nullptr, nullptr) == RTW_ERR_INVALID && rtw_trace_closest_device(s, r, -1, nullptr, &sh, nullptr) == RTW_ERR_INVALID &&
                  rtw_trace_closest_device(s, nullptr, 1, nullptr, &sh, nullptr) == RTW_ERR_INVALID && rtw_trace_occluded_device(s, r, 1, nullptr) == RTW_ERR_INVALID &&
                  rtw_trace_closest_device(s, r, (int64_t)1 << 31, nullptr, &sh, nullptr) == RTW_ERR_LIMIT && rtw_trace_closest_device(s, r, 0, nullptr, &sh, nullptr) == RTW_OK &&
                  rtw_trace_occluded_device(s, r, 0, &o) == RTW_OK;
        }
        if (!ok || !ok2) { std::fprintf(stderr, "query_main: an argument check answered wrongly (%d %d)\n", (int)ok, (int)ok2); return 2; }
    }
    for (auto& kv : scenes) CHECK(rtw_scene_destroy(kv.second));
    CHECK(rtw_context_destroy(ctx));
    std::printf("query_main ok: %d jobs\n", done);
    return 0;
}
