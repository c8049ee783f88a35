// rtw_tonemap_kernels.h -- the HDR display transform: a log-luminance histogram of the frame, an exposure adapted from it, a tone curve and the ARGB
// pack, in ONE launch that reads each accumulator entry once (rtw_tonemap / rtw_exposure_meter; the formula is the header comment of include/rtwin.h).
// Included inside rtw_device.hip's anonymous namespace after rtw_reproject_kernels.h, whose dn_lum it uses, with pack_pixel.  No operand is shared
// between pixels, so no matrix instruction fits: 16 bytes in, 20 bytes out and some sixty float operations per pixel, a kernel about memory.
//
//   tonemap_kernel<CURVE, METER, WRITE>   256 threads, a persistent grid (tonemap_blocks) whose blocks stride over chunks of TM_CHUNK = 1024 pixels.
//                              Thread t takes the pixels chunk + t + 256 j, j = 0..3: every load and store of a wave is 64 neighbouring 16-byte (ARGB: 4-byte)
//                              words, and a thread's four loads are issued before the first is used.  Nothing else touches global memory per pixel.
//                              WRITE false is rtw_exposure_meter (no curve, no store), METER false a call without an exposure object or under HOLD (no
//                              histogram, no LDS for one, no ticket).  A thread reads and then writes its own pixels only, so dst may be src.
//   the frame is mapped with the exposure the state held BEFORE the launch: the new one needs the whole frame's histogram, which no block has until the
//                              last one finishes, and a second pass over the frame is what the call exists to avoid.
//   LDS                        the gamma thresholds (1 KiB), one 256-bin histogram per wave (4 KiB: waves never contend with each other), two words.
//   a wave's histogram         a bin is the luminance's exponent and top three mantissa bits, so neighbouring pixels mostly share one.  Two ways, same
//                              integers (TonemapBufs::aggregate, option "tonemap_histogram"):
//       0  a lane per count    ds_add_u32 by every counted lane; lanes of one bin are served one after another by the LDS.
//       1  wave-aggregated     while lanes are left: the first one's bin is read with readlane, a ballot finds the lanes that share it, the first lane adds
//                              their number with a plain read-modify-write (it is alone on its wave's histogram), the lanes leave.  One trip per DISTINCT
//                              bin of the 64 pixels.  The loop is wave-uniform: every lane runs every trip.
//   after the loop             wave 0 adds the four waves' histograms, four bins per lane, and issues one global atomicAdd per bin that is not 0; ONE release
//                              fence per block; a ticket.  (The fence is an L2 write-back here and what metering costs: a fence in each of the four waves
//                              made the call 2.7 times slower at 1080p, and the grid is held to three blocks per CU for it -- tonemap_blocks.)
//   the last block             (ticket == blocks - 1) acquire fence; thread k takes bin k with atomicAdd(p, 0) and gives it back as atomicAdd(p, -value): the
//                              histogram and the ticket are zero again for the next launch, which therefore needs no memset.  Wave 0 holds four bins per lane,
//                              scans them across its lanes (six __shfl steps), clips each bin against the [lo, hi) percentile window, reduces sum k * c_k in
//                              64 bits, and lane 0 writes the new exposure, the flag and the frame count.  Then the block files the histogram as "the last
//                              metered frame's" for rtw_exposure_read.
//   across XCDs                the L2 is per XCD.  The histogram and the ticket are only ever touched by agent-scope atomics (also to read and to clear
//                              them), between a release fence in the wave that added and an acquire fence in the block that reads.  The exposure, the
//                              flag, the frame count and the filed histogram are written by the last block alone and read by later launches or copies:
//                              launch boundaries order those.  Every block reads the exposure before it takes its ticket, the last block writes it after
//                              the last ticket.
//   Vector memory operations only.

#define TM_CHUNK 1024

struct TonemapBufs {
    const float4* src;                      // (sum.xyz, int count); may be dst_accum: no __restrict__ on either
    float4* dst_accum;
    uint32_t* dst_argb;
    const float* __restrict__ gamma_thr;
    uint32_t* state;                        // rtw::EXPOSURE_* words of the exposure object; nullptr: exposure 1, no metering
    uint32_t n;                             // pixels
    float key, white, low_fraction, high_fraction, min_exposure, max_exposure, adapt;
    int aggregate;                          // the wave's histogram: 0 = a lane per count, 1 = wave-aggregated
};

// step 5 of rtwin.h: the tone curve of the exposed colour x; ww = white * white
template <int CURVE>
__device__ __forceinline__ f3 tonemap_curve(f3 x, float ww)
{
    if (CURVE == rtw::TONEMAP_REINHARD) {
        const float lx = dn_lum(x.x, x.y, x.z);
        const float s = lx > 0.0f ? (1.0f + lx / ww) / (1.0f + lx) : 1.0f;
        return mk(x.x * s, x.y * s, x.z * s);
    }
    if (CURVE == rtw::TONEMAP_ACES) {
        const float v[3] = { __builtin_fmaxf(x.x, 0.0f), __builtin_fmaxf(x.y, 0.0f), __builtin_fmaxf(x.z, 0.0f) };
        float y[3];
#pragma unroll
        for (int k = 0; k < 3; k++) y[k] = (v[k] * (2.51f * v[k] + 0.03f)) / (v[k] * (2.43f * v[k] + 0.59f) + 0.14f);
        return mk(y[0], y[1], y[2]);
    }
    return x;
}

// step 4 of rtwin.h by wave 0 of the last block: h = the frame's 256 bins in LDS; lane 0 writes the state.  Returns N (the same in every lane).
__device__ __forceinline__ uint32_t tonemap_new_exposure(const TonemapBufs& b, const uint32_t* h, uint32_t lane)
{
    uint32_t hq[4], own = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) { hq[q] = h[4 * lane + q]; own += hq[q]; }
    uint32_t inc = own;                     // inclusive scan over the lanes
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl(inc, lane >= d ? (int)(lane - d) : 0);
        if (lane >= d) inc += o;
    }
    const uint32_t N = __shfl(inc, 63);
    if (N == 0) return 0;
    uint32_t lo = (uint32_t)((double)b.low_fraction * (double)N), hi = (uint32_t)((double)b.high_fraction * (double)N);
    if (hi <= lo) { lo = 0; hi = N; }
    uint32_t P = inc - own;                 // pixels in the bins below 4 * lane
    unsigned long long S = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint32_t a = P > lo ? P : lo, e = P + hq[q] < hi ? P + hq[q] : hi;
        if (e > a) S += (unsigned long long)(4 * lane + q) * (unsigned long long)(e - a);
        P += hq[q];
    }
    for (int o = 32; o > 0; o >>= 1) S += __shfl_xor(S, o);
    const double m = (double)S / (double)(hi - lo);
    const uint32_t t = (uint32_t)(((m + 0.5) + (double)rtw::TONEMAP_BIN0) * 1048576.0);       // the window's mean bin, back to float bits: < 1112 * 2^20
    const float target = __builtin_fminf(__builtin_fmaxf(b.key / __uint_as_float(t), b.min_exposure), b.max_exposure);
    if (lane == 0) {
        const float E = __uint_as_float(b.state[rtw::EXPOSURE_VALUE]);
        b.state[rtw::EXPOSURE_VALUE] = __float_as_uint(b.state[rtw::EXPOSURE_METERED] ? E + (target - E) * b.adapt : target);
        b.state[rtw::EXPOSURE_METERED] = 1u;
        b.state[rtw::EXPOSURE_FRAMES] += 1u;
    }
    return N;
}

template <int CURVE, bool METER, bool WRITE>
__global__ __launch_bounds__(256) void tonemap_kernel(TonemapBufs b)
{
    __shared__ float thr[256];
    __shared__ uint32_t wh[4 * 256];
    __shared__ uint32_t note[2];            // [0] this block holds the last ticket, [1] N
    const uint32_t t = threadIdx.x, lane = t & 63u;
    uint32_t* const my = wh + (t >> 6) * 256u;
    if (WRITE) thr[t] = b.gamma_thr[t];
    if (METER) { wh[t] = 0u; wh[256 + t] = 0u; wh[512 + t] = 0u; wh[768 + t] = 0u; }
    const float E0 = b.state ? __uint_as_float(b.state[rtw::EXPOSURE_VALUE]) : 1.0f, ww = b.white * b.white;
    __syncthreads();
    for (uint32_t chunk = blockIdx.x * TM_CHUNK; chunk < b.n; chunk += gridDim.x * TM_CHUNK) {       // n <= 2^30, the stride < 2^23
        float4 a[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t i = chunk + t + 256u * j;
            a[j] = i < b.n ? b.src[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);        // past the frame: count 0
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t i = chunk + t + 256u * j;
            const int cnt = __float_as_int(a[j].w);
            const bool live = cnt != 0;     // a pixel of count 0 is neither counted (its luminance would be no positive finite number) nor written
            f3 c = mk(a[j].x, a[j].y, a[j].z);
            if (live && cnt != 1) { const float nf = (float)cnt; c = mk(c.x / nf, c.y / nf, c.z / nf); }      // x / 1.0f == x
            if (METER) {
                const float L = dn_lum(c.x, c.y, c.z);
                const uint32_t u = __float_as_uint(L);
                const bool counted = live && L > 0.0f && u < 0x7f800000u;
                int bin = (int)(u >> 20) - rtw::TONEMAP_BIN0;
                bin = bin < 0 ? 0 : (bin > 255 ? 255 : bin);
                if (!b.aggregate) {
                    if (counted) atomicAdd(&my[bin], 1u);
                } else {
                    unsigned long long todo = __ballot(counted);
                    while (todo) {
                        const int first = __ffsll((long long)todo) - 1;
                        const int b0 = __builtin_amdgcn_readlane(bin, first);
                        const unsigned long long same = __ballot(counted && bin == b0);
                        if ((int)lane == first) my[b0] += (uint32_t)__popcll(same);
                        todo &= ~same;
                    }
                }
            }
            if (WRITE && live) {
                const f3 y = tonemap_curve<CURVE>(mk(c.x * E0, c.y * E0, c.z * E0), ww);
                b.dst_accum[i] = make_float4(y.x, y.y, y.z, __int_as_float(1));
                b.dst_argb[i] = pack_pixel(thr, y);
            }
        }
    }
    if (!METER) return;
    __syncthreads();
    if (t < 64) {       // wave 0 files the block's bins, so that a block costs ONE release fence (an L2 write-back on this part) before its ticket
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t k = t + 64u * q, s = wh[k] + wh[256 + k] + wh[512 + k] + wh[768 + k];
            if (s) atomicAdd(&b.state[rtw::EXPOSURE_HIST + k], s);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        if (t == 0) note[0] = atomicAdd(&b.state[rtw::EXPOSURE_TICKET], 1u) == gridDim.x - 1u ? 1u : 0u;
    }
    __syncthreads();
    if (!note[0]) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const uint32_t v = atomicAdd(&b.state[rtw::EXPOSURE_HIST + t], 0u);
    atomicAdd(&b.state[rtw::EXPOSURE_HIST + t], 0u - v);
    if (t == 0) atomicAdd(&b.state[rtw::EXPOSURE_TICKET], 0u - gridDim.x);
    wh[t] = v;
    __syncthreads();
    if (t < 64) {
        const uint32_t N = tonemap_new_exposure(b, wh, lane);
        if (t == 0) note[1] = N;
    }
    __syncthreads();
    if (note[1]) b.state[rtw::EXPOSURE_LAST + t] = v;           // a frame without a counted pixel was not metered: the state stays as it is
}

// rtw_exposure_reset (clear) / rtw_exposure_set: the state's words written on the stream, so that neither needs a memset or a copy
__global__ __launch_bounds__(256) void exposure_state_kernel(uint32_t* __restrict__ state, float exposure, uint32_t metered, int clear)
{
    const uint32_t t = threadIdx.x;
    if (clear) { state[rtw::EXPOSURE_HIST + t] = 0u; state[rtw::EXPOSURE_LAST + t] = 0u; }
    if (t == 0) {
        state[rtw::EXPOSURE_VALUE] = __float_as_uint(exposure);
        state[rtw::EXPOSURE_METERED] = metered;
        if (clear) { state[rtw::EXPOSURE_TICKET] = 0u; state[rtw::EXPOSURE_FRAMES] = 0u; }
    }
}
