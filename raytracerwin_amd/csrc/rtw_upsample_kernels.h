// rtw_upsample_kernels.h -- guided (joint bilateral) upsampling: a low-resolution framebuffer carried to full size under the guidance of full-size
// feature buffers (rtw_upsample; the formula is the header comment of include/rtwin.h, its tap corner is rtw_shared.h's upsample_corner).  Included inside
// rtw_device.hip's anonymous namespace after rtw_reproject_kernels.h, whose record (RpRecord, rp_record) it uses, with DN_TARGET and pack_pixel.  A gather
// at a rational scale whose weights depend on BOTH pixels of a tap: no operand is shared between outputs, so no matrix instruction fits, and the kernel
// is about moving records.
//
//   upsample_kernel<STAGED>    ONE launch, 256 threads, a lane per full-size pixel, a block owns a 32 x 8 tile (a wave is 2 rows of 32).  A lane issues its
//                              own pixel's 40 bytes of full-size features first, so that stream is in flight while the block stages; then the tap routine
//                              (upsample_taps), the remodulation by the full-size base colour, the pack through the gamma thresholds held in LDS, and
//                              16 + 4 bytes written.  Both variants build a low pixel's record with the SAME function (rp_record, the reprojection's) and
//                              run the SAME tap routine, so a pixel's bits do not depend on which ran (-ffp-contract=off).
//     direct (STAGED false)    every tap reads its low pixel's four words from global memory (L2): 56 bytes and up to ten divisions per tap.
//     staged (STAGED true)     the low-resolution box the tile's taps can touch follows from upsample_corner of the tile's first and last pixel alone --
//                              integers, uniform over the block, no reduction and one barrier.  Round 2's ring included it is x0(first) - 1 .. x0(last) + 2
//                              clipped to the low frame; x0 is monotonic and moves by at most 31 over a tile row because w <= W, so the box is at most
//                              35 x 11 = 385 records and there is never a block that must fall back.  It is loaded once, row by row, turned into
//                              RECORDS (the divisions by the two counts and the demodulation happen once per low pixel: about 0.6 records per output at
//                              ratio 2 against 4 to 20 taps) and kept in static LDS; the taps read LDS.
//   LDS layout: colour float4 | geom float4 | key uint32 over the PW x PH box, record (i, j) at j * PW + i with the box's own PW (no padding), 36 bytes a
//   record, 13.5 KiB + the 1 KiB of gamma thresholds: room for ten blocks on a CU, which holds eight by its waves.  Bank conflicts: a 16-byte LDS read is served a quarter wave at a time and its 16
//   lanes are neighbours in one tile row; their x0 grow by 0 or 1 per lane, so they read at most 16 neighbouring records -- equal addresses are one
//   broadcast, the rest distinct banks -- for any PW.  Nothing is padded.
//   Rounds 2 and 3 are rare (a silhouette or a thin feature no bilinear tap shows).  They sit behind a lane's own branch, which a wave skips when none
//   of its lanes needs them; a lane's arithmetic is the same whichever lanes share its wave.

#define UP_TILE_W 32
#define UP_TILE_H 8
#define UP_BOX_W (UP_TILE_W + 3)        // x0(last) - x0(first) <= UP_TILE_W - 1, the bilinear pair's + 1, round 2's ring of one either side
#define UP_BOX_H (UP_TILE_H + 3)
#define UP_BOX (UP_BOX_W * UP_BOX_H)    // 385 records
#define UP_SW_MIN 1e-3f

struct UpsampleBufs {
    ReprojectFrame lo;                      // the low-resolution framebuffer and its features, w x h
    const float4* __restrict__ geom;        // the full-size features, W x H: (sum normal.xyz, sum depth)
    const float4* __restrict__ albedo;      //                               (sum rgb, int count)
    const unsigned long long* __restrict__ ids;     //                       shape in the low word
    float4* __restrict__ dst_accum;
    uint32_t* __restrict__ dst_argb;
    const float* __restrict__ gamma_thr;
    int W, H, w, h;
    float kn, kd;                           // 1 / sigma_normal^2, 1 / sigma_depth; 0 = the term is off
    uint32_t flags;                         // UPSAMPLE_DEMODULATE | UPSAMPLE_SAME_SHAPE
};

// The three rounds of one full-size pixel whose guide is gp = (n.xyz, z) and key kp = shape << 2.  fetch(qx, qy, record) hands over the record of the low
// pixel (qx, qy) and is only asked for pixels inside the low frame.  true: I is the pixel's (demodulated) value; false: no usable tap, count 0.
// A skipped tap's arithmetic may run on anything (a bad q's colour is not finite): it is selected away.
template <typename Fetch>
__device__ __forceinline__ bool upsample_taps(const UpsampleBufs& b, int x0, int y0, float tx, float ty, float4 gp, uint32_t kp, Fetch&& fetch, f3& I)
{
    const bool same_shape = (b.flags & rtw::UPSAMPLE_SAME_SHAPE) != 0, use_n = b.kn > 0.0f, use_d = b.kd > 0.0f;
    const float inv_z = use_d ? b.kd / __builtin_fmaxf(__builtin_fabsf(gp.w), 1e-6f) : 0.0f;
    float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
    auto tap = [&](int qx, int qy, float h) {
        if (qx < 0 || qx >= b.w || qy < 0 || qy >= b.h) return;
        RpRecord q;
        fetch(qx, qy, q);
        const bool take = (q.key & (RP_EMPTY | RP_BAD)) == 0 && !(same_shape && ((q.key ^ kp) >> 2) != 0);
        float e = 0.0f;
        if (use_n) { const float x = gp.x - q.g.x, y = gp.y - q.g.y, z = gp.z - q.g.z; e += (x * x + y * y + z * z) * b.kn; }
        if (use_d) { const float d = (gp.w - q.g.w) * inv_z; e += d * d; }
        const float wt = h * __builtin_amdgcn_exp2f(-(e * 1.44269504f));        // exp(-e)
        if (take) { sw += wt; sx += wt * q.c.x; sy += wt * q.c.y; sz += wt * q.c.z; }
    };
    const float wx[2] = { 1.0f - tx, tx }, wy[2] = { 1.0f - ty, ty };
#pragma unroll
    for (int k = 0; k < 4; k++) {                   // round 1: the bilinear taps
        const float bw = wx[k & 1] * wy[k >> 1];
        if (bw != 0.0f) tap(x0 + (k & 1), y0 + (k >> 1), bw);
    }
    if (sw >= UP_SW_MIN) { I = mk(sx / sw, sy / sw, sz / sw); return true; }
    sw = 0.0f; sx = 0.0f; sy = 0.0f; sz = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 2; dy++) {              // round 2: the 4 x 4 window
#pragma unroll
        for (int dx = -1; dx <= 2; dx++)
            tap(x0 + dx, y0 + dy, ((dx == 0 || dx == 1) ? 0.375f : 0.125f) * ((dy == 0 || dy == 1) ? 0.375f : 0.125f));
    }
    if (sw >= UP_SW_MIN) { I = mk(sx / sw, sy / sw, sz / sw); return true; }
    float best = -1.0f;                             // round 3: the nearest tap that holds a colour, whatever its shape
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
        const float bw = wx[k & 1] * wy[k >> 1];
        if (qx < 0 || qx >= b.w || qy < 0 || qy >= b.h) continue;
        RpRecord q;
        fetch(qx, qy, q);
        if ((q.key & (RP_EMPTY | RP_BAD)) == 0 && bw > best) { best = bw; I = mk(q.c.x, q.c.y, q.c.z); }
    }
    return best >= 0.0f;
}

template <bool STAGED>
__global__ DN_TARGET __launch_bounds__(256) void upsample_kernel(UpsampleBufs b)
{
    __shared__ float thr[256];
    __shared__ float4 lc[STAGED ? UP_BOX : 1], lg[STAGED ? UP_BOX : 1];
    __shared__ uint32_t lk[STAGED ? UP_BOX : 1];
    const int t = (int)threadIdx.x, W = b.W, H = b.H;
    thr[t] = b.gamma_thr[t];
    const int tile_x = (int)blockIdx.x * UP_TILE_W, tile_y = (int)blockIdx.y * UP_TILE_H;
    const int px = tile_x + (t & (UP_TILE_W - 1)), py = tile_y + t / UP_TILE_W;
    const bool inside = px < W && py < H, demodulate = (b.flags & rtw::UPSAMPLE_DEMODULATE) != 0;
    const int pixel = inside ? py * W + px : 0;
    // this lane's 40 bytes of the full-size stream, issued ahead of the staging
    const float4 g = b.geom[pixel], al = b.albedo[pixel];
    const uint32_t kp = (uint32_t)b.ids[pixel] << 2;
    int bx = 0, by = 0, PW = 0;
    if (STAGED) {
        // the box of the tile: the corners of its first and of its last pixel inside the frame, round 2's ring, clipped to the low frame
        const int last_x = tile_x + UP_TILE_W - 1 < W ? tile_x + UP_TILE_W - 1 : W - 1, last_y = tile_y + UP_TILE_H - 1 < H ? tile_y + UP_TILE_H - 1 : H - 1;
        int ax, ay, cx, cy; float unused;
        upsample_corner(tile_x, W, b.w, ax, unused); upsample_corner(last_x, W, b.w, cx, unused);
        upsample_corner(tile_y, H, b.h, ay, unused); upsample_corner(last_y, H, b.h, cy, unused);
        bx = ax - 1 < 0 ? 0 : ax - 1; by = ay - 1 < 0 ? 0 : ay - 1;
        cx = cx + 2 > b.w - 1 ? b.w - 1 : cx + 2; cy = cy + 2 > b.h - 1 ? b.h - 1 : cy + 2;
        PW = cx - bx + 1;
        const int n = PW * (cy - by + 1);           // <= UP_BOX because w <= W and h <= H (the call refuses anything else)
        for (int r = t; r < n; r += 256) {
            f3 mod;
            const RpRecord q = rp_record(b.lo, (by + r / PW) * b.w + bx + r % PW, demodulate, mod);
            lc[r] = q.c; lg[r] = q.g; lk[r] = q.key;
        }
    }
    __syncthreads();
    if (!inside) return;
    const int cf = __float_as_int(al.w);
    f3 I = mk(0.0f, 0.0f, 0.0f), mod = mk(1.0f, 1.0f, 1.0f);
    bool have = false;
    if (cf != 0) {
        const float nf = (float)cf;
        const float4 gp = make_float4(g.x / nf, g.y / nf, g.z / nf, g.w / nf);
        if (demodulate) mod = mk(al.x / nf + RP_EPS, al.y / nf + RP_EPS, al.z / nf + RP_EPS);
        int x0, y0; float tx, ty;
        upsample_corner(px, W, b.w, x0, tx); upsample_corner(py, H, b.h, y0, ty);
        if (STAGED)
            have = upsample_taps(b, x0, y0, tx, ty, gp, kp, [&](int qx, int qy, RpRecord& q) {
                const int r = (qy - by) * PW + (qx - bx);
                q.c = lc[r]; q.g = lg[r]; q.key = lk[r];
            }, I);
        else
            have = upsample_taps(b, x0, y0, tx, ty, gp, kp, [&](int qx, int qy, RpRecord& q) {
                f3 unused; q = rp_record(b.lo, qy * b.w + qx, demodulate, unused);
            }, I);
    }
    if (have && demodulate) I = mk(I.x * mod.x, I.y * mod.y, I.z * mod.z);
    b.dst_accum[pixel] = have ? make_float4(I.x, I.y, I.z, __int_as_float(1)) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    b.dst_argb[pixel] = pack_pixel(thr, have ? I : mk(0.0f, 0.0f, 0.0f));
}
