// indirect.cpp -- the scene RayTracerProgram::SetupScene builds (examples/default_scene.cpp) under the reference's own light, the white point light at
// (0, -4.5, 0) that Src/RayTracerScene.cpp declares and never switches on: the first-hit feature buffers of one pass, then the direct light
// (RayTracerScene::RenderLighting), one bounce of indirect light (RayTracerScene::RenderIndirect) and their sum, 4 passes each, as three PNGs:
//   OUT_direct.png    the light and its shadows: black wherever neither the light nor the sky reaches
//   OUT_indirect.png  what the lit neighbourhood and the sky send to each first hit: SAMPLES gather rays per pixel and pass (default 4)
//   OUT_sum.png       direct + indirect, the two frames' means added on the host and packed through the library's gamma thresholds
//   usage: indirect UNITYCHAN.obj WIDTH HEIGHT OUT_PREFIX [SAMPLES]
// Build: g++ -std=c++11 -Iinclude examples/indirect.cpp -Lraytracerwin_amd -lrtwin -Wl,-rpath,$PWD/raytracerwin_amd
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "RayTracerWin.hpp"

namespace {
typedef std::unique_ptr<ISurfaceMaterial> Mat;
Mat Mirror(const RVec3& c = RVec3(1, 1, 1), float fuzz = 0.0f) { return MakeUnique<SurfaceMaterial_Reflective>(c, fuzz); }
Mat Matte(const RVec3& c) { return MakeUnique<SurfaceMaterial_Diffuse>(c); }
Mat Mix(Mat a, Mat b, float f) { return MakeUnique<SurfaceMaterial_Blend>(std::move(a), std::move(b), f); }
}  // namespace

int main(int argc, char** argv)
{
    if (argc < 5) { std::fprintf(stderr, "usage: %s UNITYCHAN.obj W H OUT_PREFIX [SAMPLES]\n", argv[0]); return 2; }
    const int W = std::atoi(argv[2]), H = std::atoi(argv[3]);
    const std::string Prefix = argv[4];
    try {
        RtwDevice Device(0);
        RayTracerScene Scene(Device);
        const RVec3 gold(0.95f, 0.75f, 0.1f);
        Scene.AddShape(RSphere::Create(RVec3(1.5f, 2.5f, -2.0f), 0.9f), Mix(Mirror(), Matte(RVec3(1.0f, 0.5f, 0.1f)), 0.5f));
        Scene.AddShape(RSphere::Create(RVec3(-1.5f, -0.5f, -3.0f), 0.5f), Matte(RVec3(0.1f, 1.0f, 0.2f)));
        Scene.AddShape(RSphere::Create(RVec3(0.8f, -1.5f, -1.0f), 0.5f), Mix(Mirror(), Matte(RVec3(0.5f, 0.0f, 0.2f)), 0.5f));
        Scene.AddShape(RSphere::Create(RVec3(2.8f, -1.2f, -4.0f), 1.5f),
                       MakeUnique<SurfaceMaterial_Combine>(Mix(Mirror(gold), Matte(gold), 0.5f), MakeUnique<SurfaceMaterial_Emissive>(gold * 0.5f)));
        Scene.AddShape(RCapsule::Create(RVec3(-1.5f, -1.5f, -1.5f), RVec3(-2.0f, -1.5f, 0.0f), 0.5f),
                       Mix(Mirror(RVec3(0.8f, 0.75f, 0.6f), 0.2f), Matte(RVec3(0.25f, 0.75f, 0.6f)), 0.2f));
        Scene.AddShape(RPlane::Create(RVec3(0.0f, 1.0f, 0.0f), RVec3(0.0f, -2.0f, 0.0f)),
                       Mix(Mirror(RVec3(1, 1, 1), 0.1f), MakeUnique<SurfaceMaterial_DiffuseChecker>(), 0.5f));
        Scene.AddShape(RMeshShape::Create(argv[1]), Mix(Mirror(RVec3(1, 1, 1), 0.2f), Matte(RVec3(1.0f, 1.0f, 1.0f)), 1.0f));
        ColorBuffer Direct(Device, W, H), Indirect(Device, W, H);
        FeatureBuffers Features(Device, W, H);
        Scene.RenderFeatures(Features, 0, 1);
        const std::vector<Light> Lights(1, MakeLight(RTW_LIGHT_POINT, RVec3(0.0f, -4.5f, 0.0f), RVec3(1.0f, 1.0f, 1.0f)));
        IndirectParams Params = IndirectDefaults();
        if (argc > 5) Params.samples = std::atoi(argv[5]);
        Scene.RenderLighting(Features, Lights, LightingDefaults(), 0, 4, 12345u, Direct);
        Scene.RenderIndirect(Features, Lights, Params, 0, 4, 12345u, Indirect);
        // the sum: (sum / count) of both frames added per channel; a byte is the largest k with thresholds[k] <= c (the resolve's own pack)
        const std::vector<float> D = Direct.accuBuffer(), I = Indirect.accuBuffer();
        float Thresholds[256];
        RtwCheck(rtw_gamma_thresholds(Thresholds));
        std::vector<Pixel> Images[3] = { Direct.bitcolor(), Indirect.bitcolor(), std::vector<Pixel>((size_t)W * H) };
        for (size_t i = 0; i < (size_t)W * H; i++) {
            const float DCount = D[i * 4 + 3], ICount = I[i * 4 + 3];      // (the read-back holds the count as a float)
            Pixel Word = 0xFF000000u;
            for (int c = 0; c < 3 && DCount > 0.0f && ICount > 0.0f; c++) {
                const float v = D[i * 4 + c] / DCount + I[i * 4 + c] / ICount;
                const int Byte = v >= 1.0f ? 255 : (v > 0.0f ? std::max(0, (int)(std::upper_bound(Thresholds, Thresholds + 256, v) - Thresholds) - 1) : 0);
                Word |= (Pixel)Byte << (16 - 8 * c);
            }
            Images[2][i] = Word;
        }
        const char* Names[3] = { "_direct.png", "_indirect.png", "_sum.png" };
        for (int k = 0; k < 3; k++) {
            const std::string Path = Prefix + Names[k];
            if (rtw_png_save_argb(Path.c_str(), Images[k].data(), W, H) < 0) { std::fprintf(stderr, "cannot write %s\n", Path.c_str()); return 1; }
        }
        std::printf("wrote %s_direct.png, %s_indirect.png and %s_sum.png (%d x %d, %d gather rays)\n", Prefix.c_str(), Prefix.c_str(), Prefix.c_str(), W, H, Params.samples);
    } catch (const RtwFailure& e) {
        std::fprintf(stderr, "%s (code %d)\n", e.what(), e.code);
        return 1;
    }
    return 0;
}
