// tonemap.cpp -- the HDR display transform over an orbit of the scene RayTracerProgram::SetupScene builds (examples/default_scene.cpp): every view is
// rendered, then mapped for display by Tonemap (ACES, the exposure adapting from the previous views' log-luminance histograms) in one launch; the first
// view is metered ahead of its mapping (MeterExposure), so that it is not shown with exposure 1.  Two PNGs per view:
//   OUT_000_clipped.png      the reference's resolve: divide, clamp to [0, 1], gamma      OUT_000_tonemapped.png   the display transform
//   usage: tonemap UNITYCHAN.obj WIDTH HEIGHT VIEWS PASSES OUT_PREFIX
// Build: g++ -std=c++11 -Iinclude examples/tonemap.cpp -Lraytracerwin_amd -lrtwin -Wl,-rpath,$PWD/raytracerwin_amd
#include <cmath>
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
    if (argc < 7) { std::fprintf(stderr, "usage: %s UNITYCHAN.obj W H VIEWS PASSES OUT_PREFIX\n", argv[0]); return 2; }
    const int W = std::atoi(argv[2]), H = std::atoi(argv[3]), Views = std::atoi(argv[4]), Passes = std::atoi(argv[5]);
    const std::string Prefix = argv[6];
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
        ColorBuffer Linear(Device, W, H), Display(Device, W, H);
        Exposure Exp(Device);
        for (int View = 0; View < Views; View++) {
            const float Angle = 6.2831853f * (float)View / (float)Views;
            Scene.SetCamera(RVec3(7.0f * std::sin(Angle), 1.0f, 7.0f * std::cos(Angle)), RVec3(0, 0, -2), RVec3(0, 1, 0), 53.13f);
            Linear.Clear();
            for (int Sample = 0; Sample < Passes; Sample++)
                ThreadWorker_Render(Scene, Linear, 0, W * H - 1, 10, RenderOption(), Sample);
            if (View == 0) MeterExposure(Linear, Exp);
            Tonemap(Linear, &Exp, Display);
            int32_t Frames = 0;
            const float Next = Exp.Read(&Frames);
            ColorBuffer* Buffers[2] = { &Linear, &Display };
            const char* Names[2] = { "clipped", "tonemapped" };
            for (int k = 0; k < 2; k++) {
                char Name[48];
                std::snprintf(Name, sizeof Name, "_%03d_%s.png", View, Names[k]);
                const std::string Path = Prefix + Name;
                const std::vector<Pixel> Image = Buffers[k]->bitcolor();
                if (rtw_png_save_argb(Path.c_str(), Image.data(), W, H) < 0) { std::fprintf(stderr, "cannot write %s\n", Path.c_str()); return 1; }
            }
            std::printf("view %d: %d frames metered, the next view's exposure %.6g\n", View, Frames, Next);
        }
    } catch (const RtwFailure& e) {
        std::fprintf(stderr, "%s (code %d)\n", e.what(), e.code);
        return 1;
    }
    return 0;
}
