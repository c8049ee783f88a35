// TEST INFRASTRUCTURE: a stand-alone program over the C ABI of include/rtwin.h, linked against the objects of this directory's host build
// (the product's own sources on the HIP stand-in of shim/, AddressSanitizer + UBSan) and run directly -- nothing is preloaded.
// It runs rtw_denoise_variance under both tilings (and both prefilter routes) and rtw_reproject_moments under both stagings over wrapped buffers filled
// from files and dumps the destinations; tests/test_variance_emul.py writes the inputs and compares the dumps with tests/variance_support.py's references.
//
// usage: variance_main DIR W H [W H ...]    reads DIR/WxH.{accum,geom,albedo,ids,mu}, DIR/WxH.cams (2 x 13 floats: current, previous),
//        DIR/WxH.{cur,hist}_{accum,geom,albedo,ids} and DIR/WxH.hist_mu; writes DIR/WxH_t{0,1}.{accum,argb} and DIR/WxH_s{0,1}.{accum,argb,mu}
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>
#include "rtwin.h"

#define CHECK(call) do { const int rc_ = (int)(call); if (rc_ != 0) { std::fprintf(stderr, "variance_main: %s -> %d (%s)\n", #call, rc_, rtw_last_error()); return 2; } } while (0)

static int file_io(const std::string& path, void* data, size_t bytes, bool write)
{
    FILE* f = std::fopen(path.c_str(), write ? "wb" : "rb");
    const size_t n = f ? (write ? std::fwrite(data, 1, bytes, f) : std::fread(data, 1, bytes, f)) : 0;
    if (f) std::fclose(f);
    if (n != bytes) std::fprintf(stderr, "variance_main: cannot %s %s\n", write ? "write" : "read", path.c_str());
    return n == bytes ? 0 : 2;
}

static int dump(const std::string& out, rtw_framebuffer* dst, rtw_moments* m, size_t n)
{
    std::vector<float> a(n * 4), mu(n * 2); std::vector<uint32_t> argb(n);
    CHECK(rtw_framebuffer_read_float(dst, a.data())); CHECK(rtw_framebuffer_resolve_argb(dst, argb.data()));
    if (file_io(out + ".accum", a.data(), n * 16, true) || file_io(out + ".argb", argb.data(), n * 4, true)) return 2;
    if (m) { CHECK(rtw_moments_read(m, mu.data())); if (file_io(out + ".mu", mu.data(), n * 8, true)) return 2; }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 4 || argc % 2) { std::fprintf(stderr, "usage: variance_main DIR W H [W H ...]\n"); return 2; }
    rtw_context* ctx = nullptr;
    CHECK(rtw_context_create(0, &ctx));
    int done = 0;
    for (int k = 2; k + 1 < argc; k += 2) {
        const int W = std::atoi(argv[k]), H = std::atoi(argv[k + 1]);
        const size_t n = (size_t)W * H;
        const std::string base = std::string(argv[1]) + "/" + std::to_string(W) + "x" + std::to_string(H);
        // 0..4 the filter's sources, 5..8 the current frame, 9..13 the history and its moments, 14..16 destination accum / argb / moments, 17 a spare argb
        const char* names[14] = { ".accum", ".geom", ".albedo", ".ids", ".mu", ".cur_accum", ".cur_geom", ".cur_albedo", ".cur_ids", ".hist_accum", ".hist_geom", ".hist_albedo", ".hist_ids", ".hist_mu" };
        const size_t width[18] = { 16, 16, 16, 8, 8, 16, 16, 16, 8, 16, 16, 16, 8, 8, 16, 4, 8, 4 };
        void* dev[18];
        for (int j = 0; j < 18; j++) {
            std::vector<char> host(n * width[j], 0);
            CHECK(hipMalloc(&dev[j], host.size()));
            if (j < 14 && file_io(base + names[j], host.data(), host.size(), false)) return 2;
            CHECK(hipMemcpy(dev[j], host.data(), host.size(), hipMemcpyHostToDevice));
        }
        rtw_camera cams[2];
        if (file_io(base + ".cams", cams, sizeof cams, false)) return 2;
        rtw_framebuffer* fb[4]; rtw_features* f[3]; rtw_moments* m[3];      // source, current, history, destination
        const int fb_at[4] = { 0, 5, 9, 14 }, f_at[3] = { 1, 6, 10 }, m_at[3] = { 4, 13, 16 };
        for (int j = 0; j < 4; j++) CHECK(rtw_framebuffer_wrap(ctx, W, H, dev[fb_at[j]], dev[j == 3 ? 15 : 17], &fb[j]));
        for (int j = 0; j < 3; j++) { CHECK(rtw_features_wrap(ctx, W, H, dev[f_at[j]], dev[f_at[j] + 1], dev[f_at[j] + 2], &f[j])); CHECK(rtw_moments_wrap(ctx, W, H, dev[m_at[j]], &m[j])); }
        for (int v = 0; v <= 1; v++) {
            rtw_denoise_variance_params p; rtw_reproject_params rp;
            CHECK(rtw_denoise_variance_default_params(&p)); CHECK(rtw_reproject_default_params(&rp));
            CHECK(rtw_context_set_option(ctx, "denoise_tiling", v)); CHECK(rtw_context_set_option(ctx, "variance_prefilter", v)); CHECK(rtw_context_set_option(ctx, "reproject_staging", v));
            CHECK(rtw_denoise_variance(fb[0], f[0], m[0], &p, fb[3]));
            if (dump(base + "_t" + std::to_string(v), fb[3], nullptr, n)) return 2;
            CHECK(rtw_reproject_moments(&cams[0], &cams[1], fb[1], f[1], fb[2], f[2], m[1], &rp, 5, fb[3], m[2]));
            if (dump(base + "_s" + std::to_string(v), fb[3], m[2], n)) return 2;
            done += 2;
        }
        for (int j = 0; j < 4; j++) CHECK(rtw_framebuffer_destroy(fb[j]));
        for (int j = 0; j < 3; j++) { CHECK(rtw_features_destroy(f[j])); CHECK(rtw_moments_destroy(m[j])); }
        CHECK(rtw_context_trim(ctx));
        for (int j = 0; j < 18; j++) CHECK(hipFree(dev[j]));
    }
    CHECK(rtw_context_destroy(ctx));
    std::printf("variance_main ok: %d dumps\n", done);
    return 0;
}
