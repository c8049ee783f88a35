// TEST INFRASTRUCTURE: a stand-alone program over the C ABI of include/rtwin.h, linked against the objects of this directory's host build
// (the product's own sources on the HIP stand-in of shim/, AddressSanitizer + UBSan) and run directly -- nothing is preloaded.
// It runs the steps tests/test_tonemap_emul.py wrote into DIR/steps.txt -- the cases of tests/tonemap_support.py -- over wrapped host arrays and dumps
// after step K the destination (K.accum, K.argb) and the exposure object (K.state: exposure bits, frames, 256 bins); the test compares them with the model.
//
// usage: tonemap_main DIR
// a line of steps.txt: first-of-case frame W H mode histogram blocks curve key white low high min max adapt; DIR/<frame>.acc holds W * H float4
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "rtwin.h"

#define CHECK(call) do { const int rc_ = (call); if (rc_ < 0) { std::fprintf(stderr, "tonemap_main: %s -> %d (%s)\n", #call, rc_, rtw_last_error()); return 2; } } while (0)

template <typename T> static int dump(const std::string& path, const std::vector<T>& v)
{
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) { std::fprintf(stderr, "tonemap_main: cannot write %s\n", path.c_str()); return 2; }
    const size_t n = std::fwrite(v.data(), sizeof(T), v.size(), f);
    std::fclose(f);
    return n == v.size() ? 0 : 2;
}

int main(int argc, char** argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: tonemap_main DIR\n"); return 2; }
    const std::string dir = argv[1];
    FILE* steps = std::fopen((dir + "/steps.txt").c_str(), "r");
    if (!steps) { std::fprintf(stderr, "tonemap_main: no steps.txt\n"); return 2; }
    rtw_context* ctx = nullptr; rtw_exposure* e = nullptr;
    CHECK(rtw_context_create(0, &ctx));
    CHECK(rtw_exposure_create(ctx, &e));
    rtw_tonemap_params p;
    CHECK(rtw_tonemap_default_params(&p));
    int first, W, H, hist, blocks, done = 0;
    char frame[32], mode[32];
    while (std::fscanf(steps, "%d %31s %d %d %31s %d %d %d %f %f %f %f %f %f %f", &first, frame, &W, &H, mode, &hist, &blocks, &p.curve, &p.key, &p.white,
                       &p.low_fraction, &p.high_fraction, &p.min_exposure, &p.max_exposure, &p.adapt) == 15) {
        const size_t n = (size_t)W * H;
        std::vector<float> src(n * 4), accum(n * 4, 7.0f);
        std::vector<uint32_t> argb(n, 0x01020304u), state(258);
        FILE* in = std::fopen((dir + "/" + frame + ".acc").c_str(), "rb");
        if (!in || std::fread(src.data(), 16, n, in) != n) { std::fprintf(stderr, "tonemap_main: cannot read frame %s\n", frame); return 2; }
        std::fclose(in);
        const std::string m = mode;
        rtw_framebuffer *fs = nullptr, *fd = nullptr;
        CHECK(rtw_framebuffer_wrap(ctx, W, H, src.data(), argb.data(), &fs));       // (in place: the source's ARGB words are the destination's)
        CHECK(rtw_framebuffer_wrap(ctx, W, H, accum.data(), argb.data(), &fd));
        CHECK(rtw_context_set_option(ctx, "tonemap_histogram", hist));
        CHECK(rtw_context_set_option(ctx, "tonemap_blocks", blocks));
        if (first) CHECK(rtw_exposure_reset(e));
        p.flags = 0u;
        if (m == "hold") { CHECK(rtw_exposure_set(e, 2.5f)); p.flags = RTW_TONEMAP_HOLD; }
        if (m == "meter") CHECK(rtw_exposure_meter(fs, e, &p));
        else CHECK(rtw_tonemap(fs, m == "null" ? nullptr : e, &p, m == "inplace" ? fs : fd));
        CHECK(rtw_context_synchronize(ctx));
        float ex; int32_t frames;
        CHECK(rtw_exposure_read(e, &ex, &frames, state.data() + 2));
        std::memcpy(&state[0], &ex, 4); state[1] = (uint32_t)frames;
        const std::string base = dir + "/" + std::to_string(done++);
        if (dump(base + ".accum", m == "inplace" ? src : accum) || dump(base + ".argb", argb) || dump(base + ".state", state)) return 2;
        CHECK(rtw_framebuffer_destroy(fs));
        CHECK(rtw_framebuffer_destroy(fd));
    }
    std::fclose(steps);
    CHECK(rtw_exposure_destroy(e));
    CHECK(rtw_context_destroy(ctx));
    std::printf("tonemap_main ok: %d steps\n", done);
    return 0;
}
