// lighting.cpp -- the scene RayTracerProgram::SetupScene builds (examples/default_scene.cpp) under the reference's own light, the white point light at
// (0, -4.5, 0) that Src/RayTracerScene.cpp declares and never switches on (USE_LIGHTS 0): the first-hit feature buffers of one pass, then
// RayTracerScene::RenderLighting over them, as two PNGs:
//   OUT_hard.png      the light as a point: one shadow ray per pixel, hard shadows
//   OUT_soft.png      the light as a sphere of RADIUS (default 0.5): 4 shadow rays per pixel and pass, 4 passes, soft shadows
//   usage: lighting UNITYCHAN.obj WIDTH HEIGHT OUT_PREFIX [RADIUS]
// Build: g++ -std=c++11 -Iinclude examples/lighting.cpp -Lraytracerwin_amd -lrtwin -Wl,-rpath,$PWD/raytracerwin_amd
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
    if (argc < 5) { std::fprintf(stderr, "usage: %s UNITYCHAN.obj W H OUT_PREFIX [RADIUS]\n", argv[0]); return 2; }
    const int W = std::atoi(argv[2]), H = std::atoi(argv[3]);
    const std::string Prefix = argv[4];
    const float Radius = argc > 5 ? (float)std::atof(argv[5]) : 0.5f;
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
        ColorBuffer Hard(Device, W, H), Soft(Device, W, H);
        FeatureBuffers Features(Device, W, H);
        Scene.RenderFeatures(Features, 0, 1);
        const RVec3 Position(0.0f, -4.5f, 0.0f), White(1.0f, 1.0f, 1.0f);
        LightingParams Params = LightingDefaults();
        Scene.RenderLighting(Features, std::vector<Light>(1, MakeLight(RTW_LIGHT_POINT, Position, White)), Params, 0, 1, 12345u, Hard);
        Params.samples = 4;
        Scene.RenderLighting(Features, std::vector<Light>(1, MakeLight(RTW_LIGHT_POINT, Position, White, Radius)), Params, 0, 4, 12345u, Soft);
        ColorBuffer* Buffers[2] = { &Hard, &Soft };
        const char* Names[2] = { "_hard.png", "_soft.png" };
        for (int k = 0; k < 2; k++) {
            const std::string Path = Prefix + Names[k];
            const std::vector<Pixel> Image = Buffers[k]->bitcolor();
            if (rtw_png_save_argb(Path.c_str(), Image.data(), W, H) < 0) { std::fprintf(stderr, "cannot write %s\n", Path.c_str()); return 1; }
        }
        std::printf("wrote %s_hard.png and %s_soft.png (%d x %d, light radius %g)\n", Prefix.c_str(), Prefix.c_str(), W, H, Radius);
    } catch (const RtwFailure& e) {
        std::fprintf(stderr, "%s (code %d)\n", e.what(), e.code);
        return 1;
    }
    return 0;
}
