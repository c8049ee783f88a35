// feature_buffers.cpp -- what a denoiser or a compositor asks of a renderer before anything else: the first-hit feature buffers of the scene
// RayTracerProgram::SetupScene builds (examples/default_scene.cpp), through FeatureBuffers / RayTracerScene::RenderFeatures, as three PNGs:
//   OUT_albedo.png  the mean base colour through the reference's gamma (GetGammaSpacePixel's bytes)
//   OUT_normal.png  the mean shading normal as 0.5 n + 0.5
//   OUT_depth.png   the mean distance along the ray, scaled to the range of the pixels that hit something (near = white; the sky is black)
//   usage: feature_buffers UNITYCHAN.obj WIDTH HEIGHT PASSES OUT_PREFIX
// Build: g++ -std=c++11 -Iinclude examples/feature_buffers.cpp -Lraytracerwin_amd -lrtwin -Wl,-rpath,$PWD/raytracerwin_amd
#include <cstdio>
#include <cstdlib>
#include <string>

#include "RayTracerWin.hpp"

namespace {
typedef std::unique_ptr<ISurfaceMaterial> Mat;
Mat Mirror(const RVec3& c = RVec3(1, 1, 1), float fuzz = 0.0f) { return MakeUnique<SurfaceMaterial_Reflective>(c, fuzz); }
Mat Matte(const RVec3& c) { return MakeUnique<SurfaceMaterial_Diffuse>(c); }
Mat Mix(Mat a, Mat b, float f) { return MakeUnique<SurfaceMaterial_Blend>(std::move(a), std::move(b), f); }

UINT32 Byte(float t)            // t in [0, 1] -> 0 .. 255, rounded
{
    const int b = (int)(t * 255.0f + 0.5f);
    return (UINT32)(b < 0 ? 0 : (b > 255 ? 255 : b));
}
UINT32 GammaByte(const float* thr, float c)     // the largest k with thr[k] <= c: MakePixelColor(LinearToGamma(c)) for one channel
{
    if (!(c > 0.0f)) return 0;
    if (c >= 1.0f) return 255;
    int lo = 0, hi = 255;
    while (lo < hi) { const int mid = (lo + hi + 1) / 2; if (thr[mid] <= c) lo = mid; else hi = mid - 1; }
    return (UINT32)lo;
}
UINT32 Argb(UINT32 r, UINT32 g, UINT32 b) { return 0xFF000000u | (r << 16) | (g << 8) | b; }
}  // namespace

int main(int argc, char** argv)
{
    if (argc < 6) { std::fprintf(stderr, "usage: %s UNITYCHAN.obj W H PASSES OUT_PREFIX\n", argv[0]); return 2; }
    const int W = std::atoi(argv[2]), H = std::atoi(argv[3]), Passes = std::atoi(argv[4]);
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
        FeatureBuffers Features(Device, W, H);
        Scene.RenderFeatures(Features, 0, Passes);          // four sub-samples a pass, like the image
        std::vector<float> geom, albedo; std::vector<int32_t> ids;
        Features.Read(geom, albedo, ids);
        const size_t n = (size_t)W * H;
        // the means: sum / count in float, no division at count 1
        for (size_t i = 0; i < n; i++) {
            const float count = albedo[i * 4 + 3];
            if (count > 1.0f) for (int k = 0; k < 4; k++) { geom[i * 4 + k] = geom[i * 4 + k] / count; if (k < 3) albedo[i * 4 + k] = albedo[i * 4 + k] / count; }
        }
        float Near = 0.0f, Far = 0.0f; size_t Hits = 0;
        for (size_t i = 0; i < n; i++) {
            if (ids[i * 2] < 0) continue;
            const float d = geom[i * 4 + 3];
            if (Hits == 0 || d < Near) Near = d;
            if (Hits == 0 || d > Far) Far = d;
            Hits++;
        }
        float thr[256];
        RtwCheck(rtw_gamma_thresholds(thr));
        std::vector<UINT32> Color(n), Normal(n), Depth(n);
        for (size_t i = 0; i < n; i++) {
            Color[i] = Argb(GammaByte(thr, albedo[i * 4]), GammaByte(thr, albedo[i * 4 + 1]), GammaByte(thr, albedo[i * 4 + 2]));
            Normal[i] = Argb(Byte(geom[i * 4] * 0.5f + 0.5f), Byte(geom[i * 4 + 1] * 0.5f + 0.5f), Byte(geom[i * 4 + 2] * 0.5f + 0.5f));
            UINT32 g = 0;
            if (ids[i * 2] >= 0) g = Far > Near ? Byte((Far - geom[i * 4 + 3]) / (Far - Near)) : 255u;
            Depth[i] = Argb(g, g, g);
        }
        const char* Names[3] = { "_albedo.png", "_normal.png", "_depth.png" };
        const std::vector<UINT32>* Images[3] = { &Color, &Normal, &Depth };
        for (int k = 0; k < 3; k++) {
            const std::string Path = Prefix + Names[k];
            if (rtw_png_save_argb(Path.c_str(), Images[k]->data(), W, H) < 0) { std::fprintf(stderr, "cannot write %s\n", Path.c_str()); return 1; }
        }
        std::printf("%zu of %zu pixels hit something; distances %.9g .. %.9g\n", Hits, n, Near, Far);
    } catch (const RtwFailure& e) {
        std::fprintf(stderr, "%s (code %d)\n", e.what(), e.code);
        return 1;
    }
    return 0;
}
