// adaptive.cpp -- adaptive sampling with per-pixel pass budgets (SampleBudget, RayTracerScene::RenderPassesBudget of RayTracerWin.hpp).
// Four uniform passes go into the frame; beside them each pass is rendered alone and carried through ReprojectMoments under the unmoved camera, which
// leaves the running means of every pixel's luminance and of its square.  Then ROUNDS budgeted rounds of up to 16 passes: SampleBudget turns pass
// counts and moments into "how many more passes does this pixel need", RenderPassesBudget spends exactly those -- a sky pixel none, a contact shadow all
// sixteen -- and every pixel ends with the bits that many uniform passes would have left in it.
//   usage: adaptive MESH.obj WIDTH HEIGHT ROUNDS OUT.png
// Build: g++ -std=c++11 -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include examples/adaptive.cpp -Lraytracerwin_amd -lrtwin -L/opt/rocm/lib -lamdhip64
//        -Wl,-rpath,$PWD/raytracerwin_amd
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "RayTracerWin.hpp"

namespace {
struct DeviceArray {        // the budgets live in device memory of the caller's
    void* p;
    explicit DeviceArray(size_t bytes) : p(nullptr) { if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) throw std::runtime_error("hipMalloc failed"); }
    ~DeviceArray() { (void)hipFree(p); }
private:
    DeviceArray(const DeviceArray&); DeviceArray& operator=(const DeviceArray&);
};
}  // namespace

int main(int argc, char** argv)
{
    if (argc < 6) { std::fprintf(stderr, "usage: %s MESH.obj W H ROUNDS OUT.png\n", argv[0]); return 2; }
    const int W = std::atoi(argv[2]), H = std::atoi(argv[3]), Rounds = std::atoi(argv[4]);
    const int Depth = 4, SubSamples = 1, Warm = 4, RoundPasses = 16;
    try {
        RtwDevice Device(0);
        RayTracerScene Scene(Device);
        Scene.AddShape(RPlane::Create(RVec3(0.0f, 1.0f, 0.0f), RVec3(0.0f, -2.0f, 0.0f)), MakeUnique<SurfaceMaterial_DiffuseChecker>());
        Scene.AddShape(RMeshShape::Create(argv[1]), MakeUnique<SurfaceMaterial_Diffuse>(RVec3(1.0f, 0.9f, 0.8f)));
        const rtw_camera Camera = Scene.GetCamera();
        ColorBuffer Frame(Device, W, H), Sample(Device, W, H), History0(Device, W, H), History1(Device, W, H);
        FeatureBuffers Features0(Device, W, H), Features1(Device, W, H);
        Moments Moments0(Device, W, H), Moments1(Device, W, H);
        ColorBuffer* History[2] = { &History0, &History1 };
        FeatureBuffers* Features[2] = { &Features0, &Features1 };
        Moments* Mom[2] = { &Moments0, &Moments1 };
        Frame.Clear(); History[1]->Clear(); Features[1]->Clear(); Mom[1]->Clear();
        // the uniform passes: into the frame all at once, and one by one through the reprojection, which carries the moments
        RtwCheck(rtw_render_passes(Scene.Get(), Frame.Get(), 10, 0, 1, Depth, 0, 0, Warm, SubSamples, 12345u));
        for (int k = 0; k < Warm; k++) {
            Sample.Clear(); Features[k & 1]->Clear();
            RtwCheck(rtw_render_passes(Scene.Get(), Sample.Get(), 10, 0, 1, Depth, 0, k, 1, SubSamples, 12345u));
            Scene.RenderFeatures(*Features[k & 1], k, 1, SubSamples);
            ReprojectMoments(Camera, Camera, Sample, *Features[k & 1], *History[(k + 1) & 1], *Features[(k + 1) & 1], *Mom[(k + 1) & 1], *History[k & 1], *Mom[k & 1]);
        }
        Moments& Current = *Mom[(Warm - 1) & 1];
        DeviceArray Budget((size_t)W * H * 4);
        std::vector<int32_t> Host((size_t)W * H);
        SampleBudgetParams Params = SampleBudgetDefaults();
        Params.max_passes = RoundPasses;
        long long Spent = (long long)W * H * Warm;
        for (int Round = 0; Round < Rounds; Round++) {
            SampleBudget(Frame, Current, Budget.p, Params);       // the frame's counts have grown: a pixel that has had its share asks for nothing
            Scene.RenderPassesBudget(Frame, Budget.p, Depth, Warm + Round * RoundPasses, RoundPasses, SubSamples);
            RtwCheck(rtw_context_synchronize(Device.Get()));
            if (hipMemcpy(Host.data(), Budget.p, Host.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("hipMemcpy failed");
            long long Asked = 0;
            for (size_t i = 0; i < Host.size(); i++) Asked += Host[i];
            Spent += Asked;
            std::printf("round %d: %lld of %lld pixel passes (%.1f %%)\n", Round, Asked, (long long)W * H * RoundPasses, 100.0 * (double)Asked / ((double)W * H * RoundPasses));
        }
        std::printf("spent %lld pixel passes, a uniform render of the same depth %lld\n", Spent, (long long)W * H * (Warm + Rounds * RoundPasses));
        const std::vector<Pixel> Image = Frame.bitcolor();
        if (rtw_png_save_argb(argv[5], Image.data(), W, H) < 0) { std::fprintf(stderr, "cannot write %s\n", argv[5]); return 1; }
    } catch (const RtwFailure& e) {
        std::fprintf(stderr, "%s (code %d)\n", e.what(), e.code);
        return 1;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
