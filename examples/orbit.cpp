// orbit.cpp -- N views around a mesh: the settable camera (RayTracerScene::SetCamera) on one committed scene, one PNG per view.
//   usage: orbit MESH.obj WIDTH HEIGHT VIEWS PASSES MAXBOUNCE OUT_PREFIX      -> OUT_PREFIX_000.png, OUT_PREFIX_001.png, ...
// Build: g++ -std=c++11 -Iinclude examples/orbit.cpp -Lraytracerwin_amd -lrtwin -Wl,-rpath,$PWD/raytracerwin_amd
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "RayTracerWin.hpp"

int main(int argc, char** argv)
{
    if (argc < 8) { std::fprintf(stderr, "usage: %s MESH.obj W H VIEWS PASSES MAXBOUNCE OUT_PREFIX\n", argv[0]); return 2; }
    const int W = std::atoi(argv[2]), H = std::atoi(argv[3]), Views = std::atoi(argv[4]), Passes = std::atoi(argv[5]), MaxBounceTimes = std::atoi(argv[6]);
    const std::string Prefix = argv[7];
    try {
        RtwDevice Device(0);
        RayTracerScene Scene(Device);
        Scene.AddShape(RPlane::Create(RVec3(0, 1, 0), RVec3(0, -2, 0)), MakeUnique<SurfaceMaterial_DiffuseChecker>(RVec3(1, 1, 1), 2.0f));
        Scene.AddShape(RMeshShape::Create(argv[1]), MakeUnique<SurfaceMaterial_Diffuse>(RVec3(1.0f, 0.9f, 0.8f)));
        ColorBuffer Buffer(Device, W, H);
        const float Radius = 7.0f, Height = 2.0f;
        for (int View = 0; View < Views; View++) {
            const float Angle = 6.2831853f * (float)View / (float)Views;
            // view 0 stands where the reference's camera stands, a little higher, looking at the origin
            Scene.SetCamera(RVec3(Radius * std::sin(Angle), Height, Radius * std::cos(Angle)), RVec3(0, 0, 0), RVec3(0, 1, 0), 45.0f);
            Buffer.Clear();
            for (int Sample = 0; Sample < Passes; Sample++)
                ThreadWorker_Render(Scene, Buffer, 0, W * H - 1, MaxBounceTimes, RenderOption(), Sample);
            Device.Synchronize();
            const std::vector<Pixel> bitcolor = Buffer.bitcolor();
            char Name[32];
            std::snprintf(Name, sizeof Name, "_%03d.png", View);
            const std::string Path = Prefix + Name;
            if (!RTexture::SaveBufferToPNG(Path.c_str(), bitcolor.data(), W, H)) { std::fprintf(stderr, "cannot write %s\n", Path.c_str()); return 1; }
            const rtw_camera Cam = Scene.GetCamera();
            std::printf("view %d: eye %.9g %.9g %.9g -> %s\n", View, Cam.eye[0], Cam.eye[1], Cam.eye[2], Path.c_str());
        }
    } catch (const RtwFailure& e) {
        std::fprintf(stderr, "%s (code %d)\n", e.what(), e.code);
        return 1;
    }
    return 0;
}
