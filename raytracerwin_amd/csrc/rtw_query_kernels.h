// rtw_query_kernels.h -- ray queries on the caller's device buffers (rtw_trace_closest_device / rtw_trace_occluded_device).  Included inside
// rtw_device.hip's anonymous namespace after rtw_group_kernels.h: the walk is that file's lane_find_intersection, unchanged.
//
//   qtrace_kernel    ONE LANE PER RAY, as gtrace_kernel, but the rays come from a dense n x 7 float array and the results go to dense arrays: no
//                    GroupBufs, no lists.  A block stages the upper levels of one mesh's link tree in LDS once and its waves then take 64-ray
//                    batches in a grid-stride loop (wave w of the grid: batches w, w + waves, ...).
//                    ANY = false: FindIntersectionWithScene (Src/RayTracerScene.cpp:99-125) and the hit's shading inputs -- the record
//                    closest_kernel writes, bit for bit.  ANY = true: one byte per ray, "the closest query has a hit"; a lane stops at its
//                    first accepted test (lane_mesh_walk's ANY flag), runs no finish and keeps no carry.
//
// A batch's rays are 448 consecutive floats and its hit records 704: both cross the wave through LDS so that every global access is a
// coalesced dword per lane (element k * 64 + lane of the batch) instead of 64 strided 28- / 44-byte records.  The transposition uses the wave's
// OWN candidate-list words (entry j of thread t at cand[j * NT + t]): the lists are empty before a query starts and after it ends, so it costs no LDS
// beyond gtrace_kernel's.  Word x of the wave's slab = list entry x / 64 of lane x % 64.  A lane's stride through the slab is 7 or 11 words:
// odd, so free of bank conflicts.  With fewer than 11 list entries per lane (the 1024-thread blocks) the records cross in two halves of 32 lanes.

__device__ __forceinline__ int qslab(int x, int nt, int wbase) { return (x >> 6) * nt + wbase + (x & 63); }

template <bool STATS, bool AN, int NT, int CAP, int STAGE, bool ANY>
__global__ __launch_bounds__(NT) void qtrace_kernel(const RtwSceneDev* __restrict__ sc, const float* __restrict__ rays, uint32_t n, float* __restrict__ hits11,
                                                    int* __restrict__ shape, int* __restrict__ tri, uint8_t* __restrict__ occluded, int staged_shape, int carry_on)
{
    static_assert(CAP >= 7 && NT % 64 == 0, "a batch's 448 ray floats cross the wave through 7 list entries per lane");
    constexpr int HALVES = CAP >= 11 ? 1 : 2;       // hit records: 11 words per lane at once, or 32 lanes x 11 = 352 words (6 entries) twice
    constexpr int LPH = 64 / HALVES, KOUT = (LPH * 11 + 63) / 64;
    static_assert(KOUT <= CAP, "the hit records of one half fit the wave's list words");
    HIP_DYNAMIC_SHARED(uint32_t, gt_dyn);                 // [CAP * NT candidate words | staged records]
    uint32_t* cand = gt_dyn;
    const float4* lnodes = nullptr; int ltop = 0;
    if (STAGE) {
        const RtwShapeDev& s0 = sc->shapes[staged_shape];
        ltop = s0.tnodes_top;
        float4* dst = reinterpret_cast<float4*>(gt_dyn + CAP * NT);
        const float4* src4 = reinterpret_cast<const float4*>(s0.tnodes);
        for (int i = (int)threadIdx.x; i < ltop * 2; i += NT) dst[i] = gld4(src4, (size_t)i);
        lnodes = dst;
        __syncthreads();
    }
    const TravCtx tc = make_trav();
    const int tid = (int)threadIdx.x, lane = lane_id(), wbase = tid & ~63;
    const uint32_t n_batches = (n + 63u) >> 6;
    const uint32_t nwaves = gridDim.x * (uint32_t)(NT / 64);
    const uint32_t wave0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (uint32_t)(NT / 64) + (threadIdx.x >> 6)));
    Counters ct = { 0, 0, 0, 0, 0, 0 };
    for (uint32_t batch = wave0; batch < n_batches; batch += nwaves) {       // wave-uniform
        const uint32_t base = batch * 64u;
        const int cnt = n - base < 64u ? (int)(n - base) : 64;
        const bool have = lane < cnt;
        // ---- the batch's rays: 7 coalesced dwords per lane, then every lane picks its own 7 out of the slab (the last batch stops at n * 7 floats) ----
        const float* rb = rays + (size_t)base * 7;
#pragma unroll
        for (int k = 0; k < 7; k++) {
            const int e = k * 64 + lane;
            lstu(cand, k * NT + tid, e < cnt * 7 ? __float_as_uint(rb[e]) : 0u);
        }
        wave_lds_sync();
        float rf[7];
#pragma unroll
        for (int f = 0; f < 7; f++) rf[f] = __uint_as_float(lldu(cand, qslab(lane * 7 + f, NT, wbase)));
        wave_lds_sync();            // the walk below writes list entries
        Ray ray; ray.o = mk(0, 0, 0); ray.d = mk(0, 0, 1); ray.dist = 0.0f;
        if (have) { ray.o = mk(rf[0], rf[1], rf[2]); ray.d = mk(rf[3], rf[4], rf[5]); ray.dist = rf[6]; }
        int hs = -1, hslot = -1, cs = -1, cslot = -1; f3 pos = mk(0, 0, 0), cpos = mk(0, 0, 0); float seg = ray.dist, cdist = 0.0f;
        lane_find_intersection<STATS, AN, NT, CAP, (STAGE == 2), ANY>(sc, cand, lnodes, ltop, STAGE ? staged_shape : -1, ray, have, 0, hs, hslot, pos, seg, cs, cslot, cpos, cdist, ct);
        if (ANY) {
            if (have) occluded[(size_t)base + lane] = hs >= 0 ? (uint8_t)1 : (uint8_t)0;
            continue;
        }
        // ---- the hit's RayHitResult, by the lane that found it (group_shade_step's finish; a miss keeps RayHitResult()) ----
        Hit h; h.pos = mk(0, 0, 0); h.normal = mk(0, 0, 0); h.dist = 0.0f; h.color = mk(1, 1, 1); h.alpha = 1.0f;
        int t = -1;
        if (have && hs >= 0) {
            const RtwShapeDev& sh = sc->shapes[hs];
            if (hits11 != nullptr) {
                if (AN) {
                    hit_finish<STATS>(sc, sh, tc, pos, seg, hslot, h, t, ct);
                    // one RayHitResult serves all shapes of a query: an analytic hit with part 0 keeps the colour an earlier mesh hit sampled
                    if (carry_on && sh.kind != RTW_SHAPE_MESH && hslot == 0 && cs >= 0) {
                        Hit hc; int ti; Counters none = { 0, 0, 0, 0, 0, 0 };
                        mesh_finish<false>(sc, sc->shapes[cs], tc, cpos, cdist, cslot, hc, ti, none);
                        h.color = hc.color; h.alpha = hc.alpha;
                    }
                } else {
                    mesh_finish<STATS>(sc, sh, tc, pos, seg, hslot, h, t, ct);
                }
            } else if (tri != nullptr && (!AN || sh.kind == RTW_SHAPE_MESH)) {     // the triangle's index alone: no finish
                t = __float_as_int(gld4(reinterpret_cast<const float4*>(sh.tris), 4 * (size_t)hslot + 3).y);
            }
        }
        if (have) {
            if (shape != nullptr) shape[(size_t)base + lane] = hs;
            if (tri != nullptr) tri[(size_t)base + lane] = hs >= 0 ? t : -1;
        }
        if (hits11 != nullptr) {             // (wave-uniform)
            const float o[11] = { h.pos.x, h.pos.y, h.pos.z, h.normal.x, h.normal.y, h.normal.z, h.dist, h.color.x, h.color.y, h.color.z, h.alpha };
#pragma unroll
            for (int hf = 0; hf < HALVES; hf++) {
                const int l0 = hf * LPH;
                if (lane >= l0 && lane < l0 + LPH) {
#pragma unroll
                    for (int f = 0; f < 11; f++) lstu(cand, qslab((lane - l0) * 11 + f, NT, wbase), __float_as_uint(o[f]));
                }
                wave_lds_sync();
                const int words = (cnt - l0 < 0 ? 0 : (cnt - l0 > LPH ? LPH : cnt - l0)) * 11;
                float* hb = hits11 + ((size_t)base + (size_t)l0) * 11;
#pragma unroll
                for (int k = 0; k < KOUT; k++) {
                    const int e = k * 64 + lane;
                    if (e < words) hb[e] = __uint_as_float(lldu(cand, k * NT + tid));
                }
                wave_lds_sync();
            }
        }
    }
    if (STATS) flush_counters(sc, ct);
}
