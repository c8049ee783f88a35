// TEST INFRASTRUCTURE: a stand-alone program over the C ABI of include/rtwin.h, linked against the objects of this directory's host build
// (the product's own sources on the HIP stand-in of shim/, AddressSanitizer + UBSan) and run directly -- nothing is preloaded.
// It runs rtw_reproject over wrapped buffers filled from files, under both variants, and dumps the destination; tests/test_reproject_emul.py writes
// the inputs and compares the dumps with the reference of tests/reproject_support.py.  It also tries the calls rtw_reproject must refuse.
//
// usage: reproject_main DIR CASE [CASE ...]    reads DIR/CASE.size (W, H as int32), DIR/CASE.cams (2 x 13 floats: current, previous) and
//        DIR/CASE.{cur,hist}_{accum,geom,albedo,ids}; writes DIR/CASE_s{0,1}.{accum,argb}
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>
#include "rtwin.h"

#define CHECK(call) do { const int rc_ = (int)(call); if (rc_ != 0) { std::fprintf(stderr, "reproject_main: %s -> %d (%s)\n", #call, rc_, rtw_last_error()); return 2; } } while (0)
#define EXPECT(call, want) do { const int rc_ = (call); if (rc_ != (want)) { std::fprintf(stderr, "reproject_main: %s -> %d, expected %d\n", #call, rc_, (want)); return 2; } } while (0)

static int file_io(const std::string& path, void* data, size_t bytes, bool write)
{
    FILE* f = std::fopen(path.c_str(), write ? "wb" : "rb");
    const size_t n = f ? (write ? std::fwrite(data, 1, bytes, f) : std::fread(data, 1, bytes, f)) : 0;
    if (f) std::fclose(f);
    if (n != bytes) std::fprintf(stderr, "reproject_main: cannot %s %s\n", write ? "write" : "read", path.c_str());
    return n == bytes ? 0 : 2;
}

// the calls rtw_reproject must refuse; none of them may write the destination (cleared: all zero)
static int refusals(rtw_context* ctx)
{
    rtw_context* other = nullptr;
    CHECK(rtw_context_create(0, &other));
    rtw_framebuffer *cur = nullptr, *hist = nullptr, *dst = nullptr, *wide = nullptr, *foreign = nullptr;
    rtw_features *fc = nullptr, *fh = nullptr, *fwide = nullptr;
    CHECK(rtw_framebuffer_create(ctx, 16, 8, &cur)); CHECK(rtw_framebuffer_create(ctx, 16, 8, &hist)); CHECK(rtw_framebuffer_create(ctx, 16, 8, &dst));
    CHECK(rtw_framebuffer_create(ctx, 17, 8, &wide)); CHECK(rtw_framebuffer_create(other, 16, 8, &foreign));
    CHECK(rtw_features_create(ctx, 16, 8, &fc)); CHECK(rtw_features_create(ctx, 16, 8, &fh)); CHECK(rtw_features_create(ctx, 17, 8, &fwide));
    rtw_reproject_params ok, p;
    rtw_camera cam, c;
    CHECK(rtw_reproject_default_params(&ok)); CHECK(rtw_camera_default(&cam));
    EXPECT(rtw_reproject_default_params(nullptr), RTW_ERR_INVALID);
    EXPECT(rtw_reproject(&cam, &cam, nullptr, fc, hist, fh, &ok, dst), RTW_ERR_INVALID);
    EXPECT(rtw_reproject(&cam, &cam, cur, nullptr, hist, fh, &ok, dst), RTW_ERR_INVALID);
    EXPECT(rtw_reproject(&cam, &cam, cur, fc, nullptr, fh, &ok, dst), RTW_ERR_INVALID);
    EXPECT(rtw_reproject(&cam, &cam, cur, fc, hist, nullptr, &ok, dst), RTW_ERR_INVALID);
    EXPECT(rtw_reproject(&cam, &cam, cur, fc, hist, fh, nullptr, dst), RTW_ERR_INVALID);
    EXPECT(rtw_reproject(&cam, &cam, cur, fc, hist, fh, &ok, nullptr), RTW_ERR_INVALID);
    EXPECT(rtw_reproject(&cam, &cam, dst, fc, hist, fh, &ok, dst), RTW_ERR_INVALID);            // dst == cur
    EXPECT(rtw_reproject(&cam, &cam, cur, fc, dst, fh, &ok, dst), RTW_ERR_INVALID);             // dst == hist
    EXPECT(rtw_reproject(&cam, &cam, cur, fc, hist, fc, &ok, dst), RTW_ERR_INVALID);            // f_cur == f_hist
    EXPECT(rtw_reproject(&cam, &cam, wide, fc, hist, fh, &ok, dst), RTW_ERR_INVALID);           // sizes
    EXPECT(rtw_reproject(&cam, &cam, cur, fc, hist, fwide, &ok, dst), RTW_ERR_INVALID);
    EXPECT(rtw_reproject(&cam, &cam, cur, fc, foreign, fh, &ok, dst), RTW_ERR_INVALID);         // another context's history
    c = cam; c.focal = 0.0f; EXPECT(rtw_reproject(&c, &cam, cur, fc, hist, fh, &ok, dst), RTW_ERR_INVALID);
    c = cam; c.up[1] = 2.0f; EXPECT(rtw_reproject(&cam, &c, cur, fc, hist, fh, &ok, dst), RTW_ERR_INVALID);
    p = ok; p.depth_tolerance = std::nanf(""); EXPECT(rtw_reproject(&cam, &cam, cur, fc, hist, fh, &p, dst), RTW_ERR_INVALID);
    p = ok; p.normal_cos = std::nanf(""); EXPECT(rtw_reproject(&cam, &cam, cur, fc, hist, fh, &p, dst), RTW_ERR_INVALID);
    p = ok; p.max_history = 0; EXPECT(rtw_reproject(&cam, &cam, cur, fc, hist, fh, &p, dst), RTW_ERR_INVALID);
    p = ok; p.max_history = 65536; EXPECT(rtw_reproject(&cam, &cam, cur, fc, hist, fh, &p, dst), RTW_ERR_INVALID);
    p = ok; p.flags = 2u; EXPECT(rtw_reproject(&cam, &cam, cur, fc, hist, fh, &p, dst), RTW_ERR_INVALID);
    std::vector<float> a(16 * 8 * 4); std::vector<uint32_t> argb(16 * 8);
    CHECK(rtw_framebuffer_read_float(dst, a.data())); CHECK(rtw_framebuffer_resolve_argb(dst, argb.data()));
    for (float v : a) if (v != 0.0f) { std::fprintf(stderr, "reproject_main: a refused call wrote dst.accum\n"); return 2; }
    for (uint32_t v : argb) if (v != 0u) { std::fprintf(stderr, "reproject_main: a refused call wrote dst.argb\n"); return 2; }
    EXPECT(rtw_reproject(nullptr, nullptr, cur, fc, hist, fh, &ok, dst), RTW_OK);               // default cameras, cleared buffers: every pixel is empty
    CHECK(rtw_framebuffer_destroy(cur)); CHECK(rtw_framebuffer_destroy(hist)); CHECK(rtw_framebuffer_destroy(dst)); CHECK(rtw_framebuffer_destroy(wide));
    CHECK(rtw_framebuffer_destroy(foreign));
    CHECK(rtw_features_destroy(fc)); CHECK(rtw_features_destroy(fh)); CHECK(rtw_features_destroy(fwide));
    CHECK(rtw_context_destroy(other));
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: reproject_main DIR CASE [CASE ...]\n"); return 2; }
    const std::string dir = argv[1];
    rtw_context* ctx = nullptr;
    CHECK(rtw_context_create(0, &ctx));
    int done = 0;
    for (int k = 2; k < argc; k++) {
        const std::string base = dir + "/" + argv[k];
        int32_t size[2]; rtw_camera cams[2];
        if (file_io(base + ".size", size, sizeof size, false) || file_io(base + ".cams", cams, sizeof cams, false)) return 2;
        const int W = size[0], H = size[1];
        const size_t n = (size_t)W * H;
        std::vector<float> host(n * 4);
        const char* names[8] = { ".cur_accum", ".cur_geom", ".cur_albedo", ".cur_ids", ".hist_accum", ".hist_geom", ".hist_albedo", ".hist_ids" };
        void* dev[12];                                      // the eight sources, dst accum, dst argb, cur argb, hist argb
        for (int j = 0; j < 12; j++) CHECK(hipMalloc(&dev[j], n * ((j & 3) == 3 && j < 8 ? 8 : (j >= 9 ? 4 : 16))));
        for (int j = 0; j < 8; j++) {
            const size_t bytes = n * ((j & 3) == 3 ? 8 : 16);
            if (file_io(base + names[j], host.data(), bytes, false)) return 2;
            CHECK(hipMemcpy(dev[j], host.data(), bytes, hipMemcpyHostToDevice));
        }
        rtw_framebuffer *cur = nullptr, *hist = nullptr, *dst = nullptr; rtw_features *fc = nullptr, *fh = nullptr;
        CHECK(rtw_framebuffer_wrap(ctx, W, H, dev[0], dev[10], &cur)); CHECK(rtw_framebuffer_wrap(ctx, W, H, dev[4], dev[11], &hist));
        CHECK(rtw_framebuffer_wrap(ctx, W, H, dev[8], dev[9], &dst));
        CHECK(rtw_features_wrap(ctx, W, H, dev[1], dev[2], dev[3], &fc)); CHECK(rtw_features_wrap(ctx, W, H, dev[5], dev[6], dev[7], &fh));
        for (int staging = 0; staging <= 1; staging++) {
            rtw_reproject_params p;
            CHECK(rtw_reproject_default_params(&p));
            CHECK(rtw_context_set_option(ctx, "reproject_staging", staging));
            CHECK(rtw_reproject(&cams[0], &cams[1], cur, fc, hist, fh, &p, dst));
            std::vector<uint32_t> argb(n);
            CHECK(rtw_framebuffer_read_float(dst, host.data())); CHECK(rtw_framebuffer_resolve_argb(dst, argb.data()));
            const std::string out = base + "_s" + std::to_string(staging);
            if (file_io(out + ".accum", host.data(), n * 16, true) || file_io(out + ".argb", argb.data(), n * 4, true)) return 2;
            done++;
        }
        CHECK(rtw_framebuffer_destroy(cur)); CHECK(rtw_framebuffer_destroy(hist)); CHECK(rtw_framebuffer_destroy(dst));
        CHECK(rtw_features_destroy(fc)); CHECK(rtw_features_destroy(fh));
        for (int j = 0; j < 12; j++) CHECK(hipFree(dev[j]));
    }
    if (refusals(ctx) != 0) return 2;
    CHECK(rtw_context_destroy(ctx));
    std::printf("reproject_main ok: %d dumps, refusals checked\n", done);
    return 0;
}
