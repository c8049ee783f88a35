// TEST INFRASTRUCTURE: a stand-alone program over the C ABI of include/rtwin.h, linked against the objects of this directory's host build
// (the product's own sources on the HIP stand-in of shim/, AddressSanitizer + UBSan) and run directly -- nothing is preloaded.
// It runs rtw_upsample under both stagings over wrapped buffers filled from files and dumps the destination; tests/test_upsample_emul.py writes the
// inputs and compares the dumps with tests/upsample_support.py's reference.
//
// usage: upsample_main DIR W H w h [W H w h ...]    reads DIR/WxH.{lo_accum,lo_geom,lo_albedo,lo_ids} (w x h) and DIR/WxH.{hi_geom,hi_albedo,hi_ids};
//        writes DIR/WxH_s{0,1}.{accum,argb}
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>
#include "rtwin.h"

#define CHECK(call) do { const int rc_ = (int)(call); if (rc_ != 0) { std::fprintf(stderr, "upsample_main: %s -> %d (%s)\n", #call, rc_, rtw_last_error()); return 2; } } while (0)

static int file_io(const std::string& path, void* data, size_t bytes, bool write)
{
    FILE* f = std::fopen(path.c_str(), write ? "wb" : "rb");
    const size_t n = f ? (write ? std::fwrite(data, 1, bytes, f) : std::fread(data, 1, bytes, f)) : 0;
    if (f) std::fclose(f);
    if (n != bytes) std::fprintf(stderr, "upsample_main: cannot %s %s\n", write ? "write" : "read", path.c_str());
    return n == bytes ? 0 : 2;
}

int main(int argc, char** argv)
{
    if (argc < 6 || argc % 4 != 2) { std::fprintf(stderr, "usage: upsample_main DIR W H w h [W H w h ...]\n"); return 2; }
    rtw_context* ctx = nullptr;
    CHECK(rtw_context_create(0, &ctx));
    int done = 0;
    for (int k = 2; k + 3 < argc; k += 4) {
        const int W = std::atoi(argv[k]), H = std::atoi(argv[k + 1]), w = std::atoi(argv[k + 2]), h = std::atoi(argv[k + 3]);
        const size_t n = (size_t)W * H, m = (size_t)w * h;
        const std::string base = std::string(argv[1]) + "/" + std::to_string(W) + "x" + std::to_string(H);
        // 0..3 the low frame and its features, 4..6 the full-size features, 7..8 the destination's accum / argb, 9 the low frame's argb
        const char* names[7] = { ".lo_accum", ".lo_geom", ".lo_albedo", ".lo_ids", ".hi_geom", ".hi_albedo", ".hi_ids" };
        const size_t bytes[10] = { m * 16, m * 16, m * 16, m * 8, n * 16, n * 16, n * 8, n * 16, n * 4, m * 4 };
        void* dev[10];
        for (int j = 0; j < 10; j++) {
            std::vector<char> host(bytes[j], 0);
            CHECK(hipMalloc(&dev[j], host.size()));
            if (j < 7 && file_io(base + names[j], host.data(), host.size(), false)) return 2;
            CHECK(hipMemcpy(dev[j], host.data(), host.size(), hipMemcpyHostToDevice));
        }
        rtw_framebuffer *lo, *dst; rtw_features *f_lo, *f_hi;
        CHECK(rtw_framebuffer_wrap(ctx, w, h, dev[0], dev[9], &lo)); CHECK(rtw_framebuffer_wrap(ctx, W, H, dev[7], dev[8], &dst));
        CHECK(rtw_features_wrap(ctx, w, h, dev[1], dev[2], dev[3], &f_lo)); CHECK(rtw_features_wrap(ctx, W, H, dev[4], dev[5], dev[6], &f_hi));
        for (int v = 0; v <= 1; v++) {
            rtw_upsample_params p;
            CHECK(rtw_upsample_default_params(&p)); CHECK(rtw_context_set_option(ctx, "upsample_staging", v));
            CHECK(rtw_upsample(lo, f_lo, f_hi, &p, dst));
            std::vector<float> a(n * 4); std::vector<uint32_t> argb(n);
            CHECK(rtw_framebuffer_read_float(dst, a.data())); CHECK(rtw_framebuffer_resolve_argb(dst, argb.data()));
            const std::string out = base + "_s" + std::to_string(v);
            if (file_io(out + ".accum", a.data(), n * 16, true) || file_io(out + ".argb", argb.data(), n * 4, true)) return 2;
            done++;
        }
        CHECK(rtw_framebuffer_destroy(lo)); CHECK(rtw_framebuffer_destroy(dst)); CHECK(rtw_features_destroy(f_lo)); CHECK(rtw_features_destroy(f_hi));
        for (int j = 0; j < 10; j++) CHECK(hipFree(dev[j]));
    }
    CHECK(rtw_context_destroy(ctx));
    std::printf("upsample_main ok: %d dumps\n", done);
    return 0;
}
