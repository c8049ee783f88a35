// rtw_denoise_kernels.h -- the edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) over a framebuffer and its first-hit feature buffers
// (rtw_denoise; the formula is the header comment of include/rtwin.h).  Included inside rtw_device.hip's anonymous namespace after
// rtw_feature_kernels.h; of the rest it uses pack_pixel only.  A stencil with data-dependent weights: every tap's weight depends on BOTH of its
// pixels, so there is no shared operand for a matrix instruction, and the kernels are about moving records, not about arithmetic.
//
//   denoise_prepare_kernel   a lane per pixel: the divisions by the two counts, the demodulation, the empty / bad flags.  Writes I_0 (float4) and the
//                            guide record: (n.xyz, z) as a float4 plus a key word = shape id << 2 | DN_BAD | DN_EMPTY -- 20 bytes.  The levels read
//                            16 + 20 bytes per pixel and none of the five source arrays (the last one re-reads albedo of its own pixel to remodulate).
//   denoise_level_kernel     one level, 256 threads, an output pixel per thread, in one of three tilings; all three hand the SAME tap loop
//                            (denoise_taps) its 25 records, so a pixel's value is the same bits whichever ran (-ffp-contract=off: no fusing differs).
//     DN_DENSE    a block owns 32 x 8 pixels and stages them plus a halo of 2 * step into LDS.  Records per output: 1.69 / 2.5 / 4.5 at step 1 / 2 / 4.
//     DN_LATTICE  at step s the pixels with equal (x mod s, y mod s) are an independent lattice on which the filter is a dense 5 x 5 stencil.  A block
//                 owns, of RX = min(s, 4) lattices adjacent in x and one row phase, 64 / RX x 4 lattice points: a wave is one lattice row, its lanes run
//                 over (lattice x, lattice) with the lattice fastest, so 4 neighbouring lanes load 4 neighbouring pixels (64 bytes) and at s <= 4 a
//                 whole row of lanes loads one contiguous run.  LDS holds (64 / RX + 4) * RX x 8 records = 2.1 .. 2.5 per output at EVERY step.
//     DN_DIRECT   the dense tile at steps >= 8, where a halo of 2 * step around 32 x 8 pixels has no record two outputs share: the taps come from
//                 global memory (L2) and nothing is staged.  It exists so that "denoise_tiling" 0 means something at every step.
//   LDS layout (staged tilings): three arrays over the PW x PH records of the block, colour float4 | guide float4 | key uint32, record (i, j) at
//   j * PW + i.  A tap (dx, dy) of the thread at record c is record c + dy * SY + dx * SX with (SX, SY) = (step, step * PW) dense and (RX, PW) lattice:
//   in both, lanes that are neighbours in x read neighbouring records whatever the tap.  A 16-byte LDS read is served a quarter wave at a time;
//   16 neighbouring lanes read 256 contiguous bytes, every bank once -- no conflict for any PW, so no padding.  (Dense: a wave is 2 rows of 32
//   lanes; lattice: one row of 64.)  The key reads are 4 bytes from 64 (or 2 x 32) contiguous words: conflict-free as well.
//   The last level (LAST) remodulates, packs ARGB through the gamma thresholds held in LDS (as gsky_kernel does) and writes the destination.

// these kernels are compiled without the packed fp32 instructions (v_pk_add / mul / fma_f32): the float4 arithmetic invites them, and nothing here gains from them
#if defined(__HIP_DEVICE_COMPILE__) && __HIP_DEVICE_COMPILE__
#define DN_TARGET __attribute__((target("no-packed-fp32-ops")))
#else
#define DN_TARGET
#endif
#define DN_EMPTY 1u         // key bit: a count is 0 -- or, in LDS, the record lies outside the frame
#define DN_BAD 2u           // key bit: a channel of the pixel's colour is not finite
#define DN_EPS 1e-3f
#define DN_DENSE 0
#define DN_LATTICE 1
#define DN_DIRECT 2
#define DN_TILE_W 32
#define DN_TILE_H 8
#define DN_LAT_ROWS 4

struct DenoiseBufs {
    const float4* __restrict__ accum;       // source framebuffer: (sum.xyz, int count)
    const float4* __restrict__ geom;        // features: (sum normal.xyz, sum depth)
    const float4* __restrict__ albedo;      //           (sum rgb, int count)
    const unsigned long long* __restrict__ ids;     //   shape in the low word
    float4* __restrict__ guide;             // workspace: (n.xyz, z)
    uint32_t* __restrict__ key;             //            shape << 2 | flags
    float4* __restrict__ dst_accum;
    uint32_t* __restrict__ dst_argb;
    const float* __restrict__ gamma_thr;
    int width, height;
    uint32_t flags;                         // DENOISE_DEMODULATE | DENOISE_SAME_SHAPE
};
struct DenoiseLevel {
    const float4* __restrict__ in;          // I_i
    float4* __restrict__ out;               // I_{i+1} (unused by the last level)
    int step;
    float kc, kn, kd;                       // 1 / (sigma_color 2^-i)^2, 1 / sigma_normal^2, 1 / sigma_depth; 0 = the term is off
    int tiles_x, tiles_y;                   // lattice tiling: tiles of one lattice (group) along x / y
};

__device__ __forceinline__ bool dn_finite(float v) { return __builtin_fabsf(v) <= 3.4028235e38f; }

__global__ DN_TARGET __launch_bounds__(256) void denoise_prepare_kernel(DenoiseBufs b, float4* __restrict__ i0)
{
    const int pixel = (int)(blockIdx.x * 256 + threadIdx.x);
    if (pixel >= b.width * b.height) return;
    const float4 a = b.accum[pixel], g = b.geom[pixel], al = b.albedo[pixel];
    const int cfb = __float_as_int(a.w), cf = __float_as_int(al.w);
    uint32_t key = (uint32_t)b.ids[pixel] << 2;
    float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), gd = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (cfb == 0 || cf == 0) {
        key |= DN_EMPTY;
    } else {
        const float nfb = (float)cfb, nf = (float)cf;
        c = make_float4(a.x / nfb, a.y / nfb, a.z / nfb, 0.0f);
        gd = make_float4(g.x / nf, g.y / nf, g.z / nf, g.w / nf);
        if (!(dn_finite(c.x) && dn_finite(c.y) && dn_finite(c.z))) key |= DN_BAD;
        if (b.flags & rtw::DENOISE_DEMODULATE) { c.x = c.x / (al.x / nf + DN_EPS); c.y = c.y / (al.y / nf + DN_EPS); c.z = c.z / (al.z / nf + DN_EPS); }
    }
    i0[pixel] = c; b.guide[pixel] = gd; b.key[pixel] = key;
}

// The 25 taps of one pixel in the stated order (dy outer, dx inner).  fetch(dx, dy, colour, guide, key) hands over the record of q = p + step * (dx, dy);
// a q outside the frame comes back with DN_EMPTY.  A skipped tap's arithmetic may run on anything (a bad q's colour is not finite): it is selected away.
template <typename Fetch>
__device__ __forceinline__ void denoise_taps(const DenoiseLevel& L, bool same_shape, float4 cp, float4 gp, uint32_t kp, Fetch&& fetch, float& ox, float& oy, float& oz)
{
    const bool pbad = (kp & DN_BAD) != 0;
    const bool use_c = L.kc > 0.0f && !pbad, use_n = L.kn > 0.0f, use_d = L.kd > 0.0f;
    const float inv_z = use_d ? L.kd / __builtin_fmaxf(__builtin_fabsf(gp.w), 1e-6f) : 0.0f;
    float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const float hx = dx == 0 ? 0.375f : ((dx == 1 || dx == -1) ? 0.25f : 0.0625f), hy = dy == 0 ? 0.375f : ((dy == 1 || dy == -1) ? 0.25f : 0.0625f);
            float4 cq, gq; uint32_t kq;
            fetch(dx, dy, cq, gq, kq);
            const bool take = (kq & (DN_EMPTY | DN_BAD)) == 0 && !(same_shape && ((kq ^ kp) >> 2) != 0);
            float e = 0.0f;
            if (use_c) { const float x = cp.x - cq.x, y = cp.y - cq.y, z = cp.z - cq.z; e += (x * x + y * y + z * z) * L.kc; }
            if (use_n) { const float x = gp.x - gq.x, y = gp.y - gq.y, z = gp.z - gq.z; e += (x * x + y * y + z * z) * L.kn; }
            if (use_d) { const float d = (gp.w - gq.w) * inv_z; e += d * d; }
            const float w = (hx * hy) * __builtin_amdgcn_exp2f(-(e * 1.44269504f));       // exp(-e)
            if (take) { sw += w; sx += w * cq.x; sy += w * cq.y; sz += w * cq.z; }
        }
    }
    if (sw > 0.0f) { ox = sx / sw; oy = sy / sw; oz = sz / sw; }
    else if (!pbad) { ox = cp.x; oy = cp.y; oz = cp.z; }
    else { ox = 0.0f; oy = 0.0f; oz = 0.0f; }
}

template <int TIL, int RX, bool LAST>
__global__ DN_TARGET __launch_bounds__(256) void denoise_level_kernel(DenoiseBufs b, DenoiseLevel L)
{
    __shared__ float thr[LAST ? 256 : 1];
    if (LAST) thr[threadIdx.x] = b.gamma_thr[threadIdx.x];
    const int t = (int)threadIdx.x, W = b.width, H = b.height, step = L.step;
    const bool same_shape = (b.flags & rtw::DENOISE_SAME_SHAPE) != 0;
    int px, py;                             // this thread's pixel
    float4 cp = make_float4(0.0f, 0.0f, 0.0f, 0.0f), gp = cp; uint32_t kp = DN_EMPTY;
    float ox = 0.0f, oy = 0.0f, oz = 0.0f;
    if (TIL == DN_DIRECT) {
        px = (int)blockIdx.x * DN_TILE_W + (t & (DN_TILE_W - 1)); py = (int)blockIdx.y * DN_TILE_H + t / DN_TILE_W;
        if (LAST) __syncthreads();
        if (px >= W || py >= H) return;
        const int pixel = py * W + px;
        cp = L.in[pixel]; gp = b.guide[pixel]; kp = b.key[pixel];
        if (!(kp & DN_EMPTY))
            denoise_taps(L, same_shape, cp, gp, kp, [&](int dx, int dy, float4& cq, float4& gq, uint32_t& kq) {
                const int qx = px + step * dx, qy = py + step * dy;
                const bool in = qx >= 0 && qx < W && qy >= 0 && qy < H;
                const int q = in ? qy * W + qx : pixel;
                cq = L.in[q]; gq = b.guide[q]; kq = in ? b.key[q] : DN_EMPTY;
            }, ox, oy, oz);
    } else {
        // record (i, j) of the block's PW x PH records is the pixel (bx + i, by + j) dense, (bx + step * (i / RX) + i % RX, by + step * j) lattice
        int PW, PH, bx, by, c, SX, SY;
        if (TIL == DN_DENSE) {
            const int halo = 2 * step, tx = t & (DN_TILE_W - 1), ty = t / DN_TILE_W;
            PW = DN_TILE_W + 2 * halo; PH = DN_TILE_H + 2 * halo;
            bx = (int)blockIdx.x * DN_TILE_W - halo; by = (int)blockIdx.y * DN_TILE_H - halo;
            px = bx + halo + tx; py = by + halo + ty;
            c = (ty + halo) * PW + tx + halo; SX = step; SY = step * PW;
        } else {
            constexpr int TX = 64 / RX;
            const int lane = t & 63, wv = t >> 6;
            const int group = (int)blockIdx.x / L.tiles_x, lx0 = ((int)blockIdx.x % L.tiles_x) * TX;       // lattices group * RX .. + RX - 1
            const int ry = (int)blockIdx.y / L.tiles_y, ly0 = ((int)blockIdx.y % L.tiles_y) * DN_LAT_ROWS;
            PW = (TX + 4) * RX; PH = DN_LAT_ROWS + 4;
            bx = step * (lx0 - 2) + group * RX; by = step * (ly0 - 2) + ry;
            px = bx + step * (lane / RX + 2) + lane % RX; py = by + step * (wv + 2);
            c = (wv + 2) * PW + lane + 2 * RX; SX = RX; SY = PW;
        }
        const int N = PW * PH;
        HIP_DYNAMIC_SHARED(float4, dn_lds);                 // [N colour | N guide | N key words]
        float4* lc = dn_lds; float4* lg = dn_lds + N; uint32_t* lk = (uint32_t*)(dn_lds + 2 * N);
        for (int r = t; r < N; r += 256) {
            const int i = r % PW, j = r / PW;
            const int x = TIL == DN_DENSE ? bx + i : bx + step * (i / RX) + i % RX, y = TIL == DN_DENSE ? by + j : by + step * j;
            if (x >= 0 && x < W && y >= 0 && y < H) {
                const int q = y * W + x;
                lc[r] = L.in[q]; lg[r] = b.guide[q]; lk[r] = b.key[q];
            } else {
                lc[r] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); lg[r] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); lk[r] = DN_EMPTY;
            }
        }
        __syncthreads();
        if (px >= W || py >= H) return;
        cp = lc[c]; gp = lg[c]; kp = lk[c];
        if (!(kp & DN_EMPTY))
            denoise_taps(L, same_shape, cp, gp, kp, [&](int dx, int dy, float4& cq, float4& gq, uint32_t& kq) {
                const int q = c + dy * SY + dx * SX;
                cq = lc[q]; gq = lg[q]; kq = lk[q];
            }, ox, oy, oz);
    }
    const int pixel = py * W + px;
    if (!LAST) { L.out[pixel] = make_float4(ox, oy, oz, 0.0f); return; }
    if (!(kp & DN_EMPTY) && (b.flags & rtw::DENOISE_DEMODULATE)) {
        const float4 al = b.albedo[pixel];
        const float nf = (float)__float_as_int(al.w);
        ox = ox * (al.x / nf + DN_EPS); oy = oy * (al.y / nf + DN_EPS); oz = oz * (al.z / nf + DN_EPS);
    }
    b.dst_accum[pixel] = make_float4(ox, oy, oz, __int_as_float(1));
    b.dst_argb[pixel] = pack_pixel(thr, mk(ox, oy, oz));
}
