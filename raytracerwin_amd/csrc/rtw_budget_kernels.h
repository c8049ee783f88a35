// rtw_budget_kernels.h -- a frame's luminance moments turned into per-pixel pass budgets (rtw_sample_budget; the formula is the header comment of
// include/rtwin.h).  Included inside rtw_device.hip's anonymous namespace after rtw_reproject_kernels.h, whose Mu2 it uses.  The budget is what
// rtw_render_passes_budget reads: how many MORE passes a pixel needs before the standard error of its mean luminance falls to `tolerance` of that mean.
//
//   sample_budget_kernel<R>    ONE launch, 256 threads, a lane per pixel, a block owns a 32 x 8 tile (a wave is 2 rows of 32).  The block first turns the
//                              (32 + 2 R) x (8 + 2 R) box around its tile -- the tile and a halo of R, at most 36 x 12 = 432 pixels, two trips of the
//                              block -- into the undilated budgets b0 and keeps them in LDS as one int each: box entry r = j * PW + i, lanes that are
//                              neighbours in r are neighbours in a frame row, so the 16-byte accumulator loads and the 8-byte moment loads are contiguous
//                              runs of PW pixels.  A box entry outside the frame holds 0, which no maximum notices (every b0 is >= min_passes >= 0).  After
//                              ONE barrier a lane takes the maximum of the (2 R + 1)^2 entries around its own (R is a template argument: the window is
//                              unrolled, 1 / 9 / 25 LDS reads) and stores 4 bytes.  A halo pixel's b0 is computed by up to four blocks instead of being
//                              exchanged: 24 bytes and a division, against a second launch and a round trip through memory.
//   LDS: 432 words.  Bank conflicts: a wave's 64 lanes read two runs of 32 neighbouring words, PW apart -- two-way at worst, on 25 reads.
//   No matrix instruction fits: the work is one division per pixel and a window maximum over integers.

#define SB_TILE_W 32
#define SB_TILE_H 8
#define SB_MAX_R 2

struct BudgetBufs {
    const float4* __restrict__ accum;       // (sum rgb, int count)
    const Mu2* __restrict__ moments;        // (mu1, mu2)
    int32_t* __restrict__ budget;
    int width, height;
    float tolerance;
    int min_history, min_passes, max_passes;
};

// the undilated budget of one pixel: every operation float32 and rounded on its own (-ffp-contract=off, correctly rounded division), as rtwin.h writes it
__device__ __forceinline__ int sample_budget_b0(const BudgetBufs& b, float4 acc, Mu2 m)
{
    const int n = __float_as_int(acc.w);
    if (n < b.min_history) return b.max_passes;
    const float v = __builtin_fmaxf(m.y - m.x * m.x, 0.0f);     // (fmaxf: a NaN difference gives 0)
    const float d = b.tolerance * (m.x + 1e-3f);
    const float need = v / (d * d);
    const float x = need - (float)n;
    if (!(x < (float)b.max_passes)) return b.max_passes;        // NaN comes here
    if (x <= (float)b.min_passes) return b.min_passes;
    return (int)__builtin_ceilf(x);
}

template <int R>
__global__ __launch_bounds__(256) void sample_budget_kernel(BudgetBufs b)
{
    constexpr int PW = SB_TILE_W + 2 * R, PH = SB_TILE_H + 2 * R;
    __shared__ int box[PW * PH];
    const int t = (int)threadIdx.x, W = b.width, H = b.height;
    const int tile_x = (int)blockIdx.x * SB_TILE_W, tile_y = (int)blockIdx.y * SB_TILE_H;
    for (int r = t; r < PW * PH; r += 256) {
        const int qx = tile_x - R + r % PW, qy = tile_y - R + r / PW;
        int b0 = 0;
        if (qx >= 0 && qx < W && qy >= 0 && qy < H) {
            const size_t q = (size_t)qy * (size_t)W + (size_t)qx;
            b0 = sample_budget_b0(b, b.accum[q], b.moments[q]);
        }
        box[r] = b0;
    }
    __syncthreads();
    const int lx = t & (SB_TILE_W - 1), ly = t / SB_TILE_W;
    const int px = tile_x + lx, py = tile_y + ly;
    if (px >= W || py >= H) return;
    int most = 0;
#pragma unroll
    for (int dy = 0; dy <= 2 * R; dy++) {
#pragma unroll
        for (int dx = 0; dx <= 2 * R; dx++) {
            const int v = box[(ly + dy) * PW + lx + dx];
            most = v > most ? v : most;
        }
    }
    b.budget[(size_t)py * (size_t)W + (size_t)px] = most;
}
