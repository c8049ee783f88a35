// TEST INFRASTRUCTURE: a stand-alone program over the C ABI of include/rtwin.h, linked against the objects of this directory's host build
// (the product's own sources on the HIP stand-in of shim/, AddressSanitizer + UBSan) and run directly -- nothing is preloaded.
// It runs rtw_denoise over wrapped buffers filled from files and dumps the destination; tests/test_denoise_emul.py writes the inputs and compares
// the dumps with the reference of tests/denoise_support.py.  It also tries the calls rtw_denoise must refuse.
//
// usage: denoise_main DIR W H [W H ...]    reads DIR/WxH.{accum,geom,albedo,ids}; writes DIR/WxH_l{5,6}_t{0,1}.{accum,argb}
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>
#include "rtwin.h"

#define CHECK(call) do { const int rc_ = (int)(call); if (rc_ != 0) { std::fprintf(stderr, "denoise_main: %s -> %d (%s)\n", #call, rc_, rtw_last_error()); return 2; } } while (0)
#define EXPECT(call, want) do { const int rc_ = (call); if (rc_ != (want)) { std::fprintf(stderr, "denoise_main: %s -> %d, expected %d\n", #call, rc_, (want)); return 2; } } while (0)

static int file_io(const std::string& path, void* data, size_t bytes, bool write)
{
    FILE* f = std::fopen(path.c_str(), write ? "wb" : "rb");
    const size_t n = f ? (write ? std::fwrite(data, 1, bytes, f) : std::fread(data, 1, bytes, f)) : 0;
    if (f) std::fclose(f);
    if (n != bytes) std::fprintf(stderr, "denoise_main: cannot %s %s\n", write ? "write" : "read", path.c_str());
    return n == bytes ? 0 : 2;
}

// the calls rtw_denoise must refuse; none of them may write the destination (cleared: all zero)
static int refusals(rtw_context* ctx)
{
    rtw_context* other = nullptr;
    CHECK(rtw_context_create(0, &other));
    rtw_framebuffer *src = nullptr, *dst = nullptr, *wide = nullptr, *foreign = nullptr;
    rtw_features *f = nullptr, *fwide = nullptr;
    CHECK(rtw_framebuffer_create(ctx, 16, 8, &src)); CHECK(rtw_framebuffer_create(ctx, 16, 8, &dst)); CHECK(rtw_framebuffer_create(ctx, 17, 8, &wide));
    CHECK(rtw_framebuffer_create(other, 16, 8, &foreign));
    CHECK(rtw_features_create(ctx, 16, 8, &f)); CHECK(rtw_features_create(ctx, 17, 8, &fwide));
    rtw_denoise_params ok, p;
    CHECK(rtw_denoise_default_params(&ok));
    EXPECT(rtw_denoise_default_params(nullptr), RTW_ERR_INVALID);
    EXPECT(rtw_denoise(nullptr, f, &ok, dst), RTW_ERR_INVALID);
    EXPECT(rtw_denoise(src, nullptr, &ok, dst), RTW_ERR_INVALID);
    EXPECT(rtw_denoise(src, f, nullptr, dst), RTW_ERR_INVALID);
    EXPECT(rtw_denoise(src, f, &ok, nullptr), RTW_ERR_INVALID);
    EXPECT(rtw_denoise(src, f, &ok, src), RTW_ERR_INVALID);             // dst == src
    EXPECT(rtw_denoise(wide, f, &ok, dst), RTW_ERR_INVALID);            // sizes
    EXPECT(rtw_denoise(src, fwide, &ok, dst), RTW_ERR_INVALID);
    EXPECT(rtw_denoise(foreign, f, &ok, dst), RTW_ERR_INVALID);         // another context's source
    p = ok; p.levels = 0; EXPECT(rtw_denoise(src, f, &p, dst), RTW_ERR_INVALID);
    p = ok; p.levels = 7; EXPECT(rtw_denoise(src, f, &p, dst), RTW_ERR_INVALID);
    p = ok; p.sigma_normal = std::nanf(""); EXPECT(rtw_denoise(src, f, &p, dst), RTW_ERR_INVALID);
    p = ok; p.flags = 4u; EXPECT(rtw_denoise(src, f, &p, dst), RTW_ERR_INVALID);
    std::vector<float> a(16 * 8 * 4); std::vector<uint32_t> argb(16 * 8);
    CHECK(rtw_framebuffer_read_float(dst, a.data())); CHECK(rtw_framebuffer_resolve_argb(dst, argb.data()));
    for (float v : a) if (v != 0.0f) { std::fprintf(stderr, "denoise_main: a refused call wrote dst.accum\n"); return 2; }
    for (uint32_t v : argb) if (v != 0u) { std::fprintf(stderr, "denoise_main: a refused call wrote dst.argb\n"); return 2; }
    EXPECT(rtw_denoise(src, f, &ok, dst), RTW_OK);                      // cleared buffers: every pixel is empty
    CHECK(rtw_framebuffer_destroy(src)); CHECK(rtw_framebuffer_destroy(dst)); CHECK(rtw_framebuffer_destroy(wide)); CHECK(rtw_framebuffer_destroy(foreign));
    CHECK(rtw_features_destroy(f)); CHECK(rtw_features_destroy(fwide));
    CHECK(rtw_context_destroy(other));
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 4 || argc % 2) { std::fprintf(stderr, "usage: denoise_main DIR W H [W H ...]\n"); return 2; }
    const std::string dir = argv[1];
    rtw_context* ctx = nullptr;
    CHECK(rtw_context_create(0, &ctx));
    int done = 0;
    for (int k = 2; k + 1 < argc; k += 2) {
        const int W = std::atoi(argv[k]), H = std::atoi(argv[k + 1]);
        const size_t n = (size_t)W * H;
        const std::string base = dir + "/" + std::to_string(W) + "x" + std::to_string(H);
        std::vector<float> host(n * 4);
        const char* names[4] = { ".accum", ".geom", ".albedo", ".ids" };
        void* dev[7];                                       // accum, geom, albedo, ids, dst accum, dst argb, src argb
        for (int j = 0; j < 7; j++) CHECK(hipMalloc(&dev[j], n * (j == 3 ? 8 : (j >= 5 ? 4 : 16))));
        for (int j = 0; j < 4; j++) {
            const size_t bytes = n * (j == 3 ? 8 : 16);
            if (file_io(base + names[j], host.data(), bytes, false)) return 2;
            CHECK(hipMemcpy(dev[j], host.data(), bytes, hipMemcpyHostToDevice));
        }
        rtw_framebuffer *src = nullptr, *dst = nullptr; rtw_features* f = nullptr;
        CHECK(rtw_framebuffer_wrap(ctx, W, H, dev[0], dev[6], &src));
        CHECK(rtw_framebuffer_wrap(ctx, W, H, dev[4], dev[5], &dst));
        CHECK(rtw_features_wrap(ctx, W, H, dev[1], dev[2], dev[3], &f));
        for (int levels = 5; levels <= 6; levels++) for (int tiling = 0; tiling <= 1; tiling++) {
            rtw_denoise_params p;
            CHECK(rtw_denoise_default_params(&p));
            p.levels = levels;
            CHECK(rtw_context_set_option(ctx, "denoise_tiling", tiling));
            CHECK(rtw_denoise(src, f, &p, dst));
            std::vector<uint32_t> argb(n);
            CHECK(rtw_framebuffer_read_float(dst, host.data())); CHECK(rtw_framebuffer_resolve_argb(dst, argb.data()));
            const std::string out = base + "_l" + std::to_string(levels) + "_t" + std::to_string(tiling);
            if (file_io(out + ".accum", host.data(), n * 16, true) || file_io(out + ".argb", argb.data(), n * 4, true)) return 2;
            done++;
        }
        CHECK(rtw_framebuffer_destroy(src)); CHECK(rtw_framebuffer_destroy(dst)); CHECK(rtw_features_destroy(f));
        CHECK(rtw_context_trim(ctx));
        for (int j = 0; j < 7; j++) CHECK(hipFree(dev[j]));
    }
    if (refusals(ctx) != 0) return 2;
    CHECK(rtw_context_destroy(ctx));
    std::printf("denoise_main ok: %d dumps, refusals checked\n", done);
    return 0;
}
