// upsample.cpp -- the SVGF loop of examples/svgf.cpp at HALF the frame, carried to full size by full-size features: each frame is rendered at one
// sample per pixel at WIDTH/2 x HEIGHT/2, reprojected with its moments and filtered there; then one feature frame at WIDTH x HEIGHT guides Upsample
// (RayTracerWin.hpp), which remodulates with the full-size base colour, so textures and silhouettes are full resolution.  Beside it the same frame through
// the same chain at full size.  For the last frame two PNGs:
//   OUT_upsampled.png   render, reproject, filter at half size -> features at full size -> Upsample
//   OUT_full.png        render, reproject, filter at full size
//   usage: upsample UNITYCHAN.obj WIDTH HEIGHT FRAMES OUT_PREFIX        (WIDTH and HEIGHT even)
// Build: g++ -std=c++11 -Iinclude examples/upsample.cpp -Lraytracerwin_amd -lrtwin -Wl,-rpath,$PWD/raytracerwin_amd
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
// the buffers of one SVGF chain at one size, and a frame of it: render, features, reprojection with moments, the variance-guided filter into Clean
struct Chain {
    int W, H;
    ColorBuffer Sample, History0, History1, Clean;
    FeatureBuffers Features0, Features1;
    Moments Moments0, Moments1;
    Chain(RtwDevice& Device, int w, int h) : W(w), H(h), Sample(Device, w, h), History0(Device, w, h), History1(Device, w, h), Clean(Device, w, h),
        Features0(Device, w, h), Features1(Device, w, h), Moments0(Device, w, h), Moments1(Device, w, h) { History1.Clear(); Features1.Clear(); Moments1.Clear(); }
    FeatureBuffers& Features(int Frame) { return Frame & 1 ? Features1 : Features0; }
    void Step(RayTracerScene& Scene, int Frame, const rtw_camera& Current, const rtw_camera& Previous)
    {
        ColorBuffer &Old = Frame & 1 ? History0 : History1, &New = Frame & 1 ? History1 : History0;
        Moments &OldMoments = Frame & 1 ? Moments0 : Moments1, &NewMoments = Frame & 1 ? Moments1 : Moments0;
        Sample.Clear(); Features(Frame).Clear();
        RtwCheck(rtw_render_passes(Scene.Get(), Sample.Get(), 10, 0, 1, 4, 0, Frame, 1, 1, 12345u));       // pass `Frame`: one sample, depth 4
        Scene.RenderFeatures(Features(Frame), Frame, 1, 1);
        ReprojectMoments(Current, Previous, Sample, Features(Frame), Old, Features(Frame + 1), OldMoments, New, NewMoments);
        DenoiseVariance(New, Features(Frame), NewMoments, Clean);
    }
};
}  // namespace

int main(int argc, char** argv)
{
    if (argc < 6) { std::fprintf(stderr, "usage: %s UNITYCHAN.obj W H FRAMES OUT_PREFIX\n", argv[0]); return 2; }
    const int W = std::atoi(argv[2]), H = std::atoi(argv[3]), Frames = std::atoi(argv[4]);
    const std::string Prefix = argv[5];
    if (W < 2 || H < 2 || (W | H) & 1 || Frames < 1) { std::fprintf(stderr, "W and H must be even, FRAMES at least 1\n"); return 2; }
    try {
        RtwDevice Device(0);
        RayTracerScene Scene(Device);
        const RVec3 gold(0.95f, 0.75f, 0.1f);
        Scene.AddShape(RSphere::Create(RVec3(1.5f, 2.5f, -2.0f), 0.9f), Mix(Mirror(), Matte(RVec3(1.0f, 0.5f, 0.1f)), 0.5f));
        Scene.AddShape(RSphere::Create(RVec3(-1.5f, -0.5f, -3.0f), 0.5f), Matte(RVec3(0.1f, 1.0f, 0.2f)));
        Scene.AddShape(RSphere::Create(RVec3(2.8f, -1.2f, -4.0f), 1.5f),
                       MakeUnique<SurfaceMaterial_Combine>(Mix(Mirror(gold), Matte(gold), 0.5f), MakeUnique<SurfaceMaterial_Emissive>(gold * 0.5f)));
        Scene.AddShape(RPlane::Create(RVec3(0.0f, 1.0f, 0.0f), RVec3(0.0f, -2.0f, 0.0f)),
                       Mix(Mirror(RVec3(1, 1, 1), 0.1f), MakeUnique<SurfaceMaterial_DiffuseChecker>(), 0.5f));
        Scene.AddShape(RMeshShape::Create(argv[1]), Mix(Mirror(RVec3(1, 1, 1), 0.2f), Matte(RVec3(1.0f, 1.0f, 1.0f)), 1.0f));
        Chain Half(Device, W / 2, H / 2), Full(Device, W, H);
        FeatureBuffers Guide(Device, W, H);
        ColorBuffer Upsampled(Device, W, H);
        rtw_camera Previous = Scene.GetCamera();
        for (int Frame = 0; Frame < Frames; Frame++) {
            const float Angle = 0.02f * (float)Frame;           // about a degree a frame, on the reference camera's circle
            Scene.SetCamera(RVec3(7.0f * std::sin(Angle), 0.0f, 7.0f * std::cos(Angle)), RVec3(0, 0, 0), RVec3(0, 1, 0), 53.130102f);
            const rtw_camera Current = Scene.GetCamera();
            Half.Step(Scene, Frame, Current, Previous);
            Guide.Clear();
            Scene.RenderFeatures(Guide, Frame, 1, 1);           // the only full-size work of the half-size route besides Upsample itself
            Upsample(Half.Clean, Half.Features(Frame), Guide, Upsampled);
            Full.Step(Scene, Frame, Current, Previous);
            Previous = Current;
        }
        if (!Save(Upsampled, Prefix + "_upsampled.png", W, H) || !Save(Full.Clean, Prefix + "_full.png", W, H)) return 1;
        std::printf("wrote %s_upsampled.png (filtered at %d x %d) and %s_full.png (%d x %d) after %d frames\n", Prefix.c_str(), W / 2, H / 2, Prefix.c_str(), W, H, Frames);
    } catch (const RtwFailure& e) {
        std::fprintf(stderr, "%s (code %d)\n", e.what(), e.code);
        return 1;
    }
    return 0;
}
