// depth_of_field.cpp -- a focus pull: N frames of a mesh above a checker plane through a thin lens (RayTracerScene::SetLens) whose focus distance
// steps from near to far on one committed scene, one PNG per frame.
//   usage: depth_of_field MESH.obj WIDTH HEIGHT FRAMES PASSES MAXBOUNCE OUT_PREFIX      -> OUT_PREFIX_000.png, OUT_PREFIX_001.png, ...
// Build: g++ -std=c++11 -Iinclude examples/depth_of_field.cpp -Lraytracerwin_amd -lrtwin -Wl,-rpath,$PWD/raytracerwin_amd
#include <cstdio>
#include <cstdlib>
#include <string>

#include "RayTracerWin.hpp"

int main(int argc, char** argv)
{
    if (argc < 8) { std::fprintf(stderr, "usage: %s MESH.obj W H FRAMES PASSES MAXBOUNCE OUT_PREFIX\n", argv[0]); return 2; }
    const int W = std::atoi(argv[2]), H = std::atoi(argv[3]), Frames = std::atoi(argv[4]), Passes = std::atoi(argv[5]), MaxBounceTimes = std::atoi(argv[6]);
    const std::string Prefix = argv[7];
    try {
        RtwDevice Device(0);
        RayTracerScene Scene(Device);
        Scene.AddShape(RPlane::Create(RVec3(0, 1, 0), RVec3(0, -2, 0)), MakeUnique<SurfaceMaterial_DiffuseChecker>(RVec3(1, 1, 1), 2.0f));
        Scene.AddShape(RMeshShape::Create(argv[1]), MakeUnique<SurfaceMaterial_Diffuse>(RVec3(1.0f, 0.9f, 0.8f)));
        Scene.SetCamera(RVec3(0, 1.5f, 7), RVec3(0, 0, 0), RVec3(0, 1, 0), 45.0f);
        ColorBuffer Buffer(Device, W, H);
        // the mesh sits about 7.2 from the eye: the focus travels from in front of it to the plane far behind it
        const float Aperture = 0.15f, Near = 4.0f, Far = 16.0f;
        for (int Frame = 0; Frame < Frames; Frame++) {
            const float Focus = Frames > 1 ? Near + (Far - Near) * (float)Frame / (float)(Frames - 1) : Near;
            Scene.SetLens(Aperture, Focus);
            Buffer.Clear();
            for (int Sample = 0; Sample < Passes; Sample++)
                ThreadWorker_Render(Scene, Buffer, 0, W * H - 1, MaxBounceTimes, RenderOption(), Sample);
            Device.Synchronize();
            const std::vector<Pixel> bitcolor = Buffer.bitcolor();
            char Name[32];
            std::snprintf(Name, sizeof Name, "_%03d.png", Frame);
            const std::string Path = Prefix + Name;
            if (!RTexture::SaveBufferToPNG(Path.c_str(), bitcolor.data(), W, H)) { std::fprintf(stderr, "cannot write %s\n", Path.c_str()); return 1; }
            std::printf("focus %.9g -> %s\n", Scene.GetLens().focus_distance, Path.c_str());
        }
    } catch (const RtwFailure& e) {
        std::fprintf(stderr, "%s (code %d)\n", e.what(), e.code);
        return 1;
    }
    return 0;
}
