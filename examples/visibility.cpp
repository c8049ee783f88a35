// visibility.cpp -- closest-hit and any-hit queries on device buffers: the camera rays of a small frame, then one shadow ray per hit towards a
// point light; an ARGB PNG in three flat colours (sky, lit, shadowed) and the three counts.
//   usage: visibility MESH.obj WIDTH HEIGHT OUT.png
// Build: g++ -std=c++11 -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include examples/visibility.cpp -Lraytracerwin_amd -lrtwin -L/opt/rocm/lib -lamdhip64
//        -Wl,-rpath,$PWD/raytracerwin_amd
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "RayTracerWin.hpp"

struct DeviceArray {        // plain device memory, the caller's (as a torch tensor would be)
    void* p;
    explicit DeviceArray(size_t bytes) : p(nullptr) { if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) throw std::runtime_error("hipMalloc failed"); }
    ~DeviceArray() { (void)hipFree(p); }
private:
    DeviceArray(const DeviceArray&); DeviceArray& operator=(const DeviceArray&);
};
static void Copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) { if (bytes && hipMemcpy(dst, src, bytes, kind) != hipSuccess) throw std::runtime_error("hipMemcpy failed"); }

int main(int argc, char** argv)
{
    if (argc < 5) { std::fprintf(stderr, "usage: %s MESH.obj W H OUT.png\n", argv[0]); return 2; }
    const int W = std::atoi(argv[2]), H = std::atoi(argv[3]);
    const float Light[3] = { 4.0f, 6.0f, 5.0f };
    try {
        RtwDevice Device(0);
        RayTracerScene Scene(Device);
        Scene.AddShape(RPlane::Create(RVec3(0, 1, 0), RVec3(0, -2, 0)), MakeUnique<SurfaceMaterial_DiffuseChecker>(RVec3(1, 1, 1), 2.0f));
        Scene.AddShape(RMeshShape::Create(argv[1]), MakeUnique<SurfaceMaterial_Diffuse>(RVec3(1.0f, 0.9f, 0.8f)));
        Scene.Commit();
        // the camera rays of every pixel (pass 0, sub-sample 0), made on the host and uploaded once
        const int64_t N = (int64_t)W * H;
        std::vector<int32_t> Pixels((size_t)N);
        for (int64_t i = 0; i < N; i++) Pixels[(size_t)i] = (int32_t)i;
        std::vector<float> Rays((size_t)N * 7);
        const rtw_camera Cam = Scene.GetCamera();
        RtwCheck(rtw_camera_rays(&Cam, W, H, Pixels.data(), N, 0, 0, 12345u, Rays.data()));
        DeviceArray dRays((size_t)N * 28), dHits((size_t)N * 44), dShape((size_t)N * 4);
        Copy(dRays.p, Rays.data(), (size_t)N * 28, hipMemcpyHostToDevice);
        Scene.FindIntersectionsDevice(dRays.p, N, dHits.p, dShape.p, nullptr);
        Device.Synchronize();
        std::vector<float> Hits((size_t)N * 11);
        std::vector<int32_t> Shape((size_t)N);
        Copy(Hits.data(), dHits.p, (size_t)N * 44, hipMemcpyDeviceToHost);
        Copy(Shape.data(), dShape.p, (size_t)N * 4, hipMemcpyDeviceToHost);
        // one shadow ray per hit: from just above the surface towards the light, as long as the way there
        std::vector<float> Shadow; std::vector<int64_t> Owner;
        for (int64_t i = 0; i < N; i++) {
            if (Shape[(size_t)i] < 0) continue;
            const float* h = &Hits[(size_t)i * 11];
            float o[3], d[3];
            for (int k = 0; k < 3; k++) { o[k] = h[k] + h[3 + k] * 1e-3f; d[k] = Light[k] - o[k]; }
            const float Len = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
            const float r[7] = { o[0], o[1], o[2], d[0] / Len, d[1] / Len, d[2] / Len, Len };
            Shadow.insert(Shadow.end(), r, r + 7);
            Owner.push_back(i);
        }
        const int64_t M = (int64_t)Owner.size();
        std::vector<unsigned char> Occluded((size_t)M);
        if (M > 0) {
            DeviceArray dShadow((size_t)M * 28), dOccluded((size_t)M);
            Copy(dShadow.p, Shadow.data(), (size_t)M * 28, hipMemcpyHostToDevice);
            Scene.OccludedDevice(dShadow.p, M, dOccluded.p);
            Device.Synchronize();
            Copy(Occluded.data(), dOccluded.p, (size_t)M, hipMemcpyDeviceToHost);
        }
        std::vector<Pixel> Image((size_t)N, MakeUint32Color(110, 160, 230, 255));       // sky
        int64_t Lit = 0, Shadowed = 0;
        for (int64_t j = 0; j < M; j++) {
            if (Occluded[(size_t)j]) { Shadowed++; Image[(size_t)Owner[(size_t)j]] = MakeUint32Color(40, 40, 60, 255); }
            else { Lit++; Image[(size_t)Owner[(size_t)j]] = MakeUint32Color(250, 240, 200, 255); }
        }
        if (!RTexture::SaveBufferToPNG(argv[4], Image.data(), W, H)) { std::fprintf(stderr, "cannot write %s\n", argv[4]); return 1; }
        std::printf("sky %lld lit %lld shadowed %lld -> %s\n", (long long)(N - M), (long long)Lit, (long long)Shadowed, argv[4]);
    } catch (const RtwFailure& e) {
        std::fprintf(stderr, "%s (code %d)\n", e.what(), e.code);
        return 1;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
