// svgf.cpp -- the orbit of examples/temporal.cpp through the whole chain: each frame is rendered at ONE sample per pixel with its first-hit features,
// reprojected onto the accumulated history WITH its luminance moments (ReprojectMoments of RayTracerWin.hpp: two history buffers, two feature objects
// and two moments objects, swapped each frame), then filtered under the guidance of the variance those moments give (DenoiseVariance).  Per frame two PNGs:
//   OUT_NNN_svgf.png    render -> reproject with moments -> variance-guided filter
//   OUT_NNN_fixed.png   the same reprojected frame through Denoise, one fixed sigma_color for converged and disoccluded pixels alike
//   usage: svgf UNITYCHAN.obj WIDTH HEIGHT FRAMES OUT_PREFIX
// Build: g++ -std=c++11 -Iinclude examples/svgf.cpp -Lraytracerwin_amd -lrtwin -Wl,-rpath,$PWD/raytracerwin_amd
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
bool Save(ColorBuffer& Buffer, const std::string& Path, int W, int H)
{
    const std::vector<Pixel> Image = Buffer.bitcolor();
    if (rtw_png_save_argb(Path.c_str(), Image.data(), W, H) >= 0) return true;
    std::fprintf(stderr, "cannot write %s\n", Path.c_str());
    return false;
}
}  // namespace

int main(int argc, char** argv)
{
    if (argc < 6) { std::fprintf(stderr, "usage: %s UNITYCHAN.obj W H FRAMES OUT_PREFIX\n", argv[0]); return 2; }
    const int W = std::atoi(argv[2]), H = std::atoi(argv[3]), Frames = std::atoi(argv[4]);
    const std::string Prefix = argv[5];
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
        ColorBuffer Sample(Device, W, H), History0(Device, W, H), History1(Device, W, H), Clean(Device, W, H);
        FeatureBuffers Features0(Device, W, H), Features1(Device, W, H);
        ColorBuffer* History[2] = { &History0, &History1 };
        FeatureBuffers* Features[2] = { &Features0, &Features1 };
        Moments Moments0(Device, W, H), Moments1(Device, W, H);
        Moments* Mom[2] = { &Moments0, &Moments1 };
        History[1]->Clear(); Features[1]->Clear(); Mom[1]->Clear();     // frame 0 reads them: a cleared history means "no history"
        rtw_camera Previous = Scene.GetCamera();
        for (int Frame = 0; Frame < Frames; Frame++) {
            const float Angle = 0.02f * (float)Frame;           // about a degree a frame, on the reference camera's circle
            Scene.SetCamera(RVec3(7.0f * std::sin(Angle), 0.0f, 7.0f * std::cos(Angle)), RVec3(0, 0, 0), RVec3(0, 1, 0), 53.130102f);
            const rtw_camera Current = Scene.GetCamera();
            ColorBuffer &Old = *History[(Frame + 1) & 1], &New = *History[Frame & 1];
            FeatureBuffers &Now = *Features[Frame & 1], &Before = *Features[(Frame + 1) & 1];
            Sample.Clear(); Now.Clear();
            RtwCheck(rtw_render_passes(Scene.Get(), Sample.Get(), 10, 0, 1, 4, 0, Frame, 1, 1, 12345u));       // pass `Frame`: one sample, depth 4
            Scene.RenderFeatures(Now, Frame, 1, 1);
            ReprojectMoments(Current, Previous, Sample, Now, Old, Before, *Mom[(Frame + 1) & 1], New, *Mom[Frame & 1]);
            char Number[16];
            std::snprintf(Number, sizeof Number, "_%03d", Frame);
            DenoiseVariance(New, Now, *Mom[Frame & 1], Clean);
            if (!Save(Clean, Prefix + Number + "_svgf.png", W, H)) return 1;
            Denoise(New, Now, Clean);
            if (!Save(Clean, Prefix + Number + "_fixed.png", W, H)) return 1;
            Previous = Current;
        }
        std::printf("wrote %d pairs %s_NNN_svgf.png / %s_NNN_fixed.png (%d x %d)\n", Frames, Prefix.c_str(), Prefix.c_str(), W, H);
    } catch (const RtwFailure& e) {
        std::fprintf(stderr, "%s (code %d)\n", e.what(), e.code);
        return 1;
    }
    return 0;
}
