// rtw_variance_kernels.h -- the variance-guided a-trous filter (the spatial half of SVGF, Schied et al. 2017) over a reprojected framebuffer, its
// first-hit feature buffers and its luminance moments (rtw_denoise_variance; the formula is the header comment of include/rtwin.h).  Included inside
// rtw_device.hip's anonymous namespace after rtw_reproject_kernels.h: it uses rtw_denoise_kernels.h's DenoiseBufs, DenoiseLevel, tilings and key bits,
// rtw_reproject_kernels.h's Mu2 and dn_lum, and pack_pixel.  The structure is rtw_denoise's, the kernels are their own, so that rtw_denoise's
// instantiations stay what they were.  As there, every tap's weight depends on both of its pixels: no matrix instruction fits.
//
//   variance_estimate_kernel   prepare and estimate in ONE launch, 256 threads, a block owns a 32 x 8 tile, a lane a pixel.  A lane makes its pixel's
//                              record as denoise_prepare_kernel does (the same arithmetic: I_0, guide, key) and reads its moments.  The variance goes
//                              into the FOURTH WORD of I_0, free in rtw_denoise: at every level the variance travels with the colour, in the same
//                              16-byte loads and LDS records, and costs no traffic of its own.
//                              A pixel with N >= min_history takes V_0 from its own moments.  The 7 x 7 spatial fallback is decided PER BLOCK: the
//                              lanes raise a flag in LDS when they are short of history, and only a block with such a lane stages its tile plus a halo
//                              of 3 -- 38 x 14 records of (guide float4, moments, key) = 28 bytes, 14.5 KiB static LDS -- making each halo record from
//                              the source arrays with the lane's own routine.  After a few unmoved frames no block stages anything and the launch costs
//                              what denoise_prepare_kernel costs plus 8 bytes per pixel.  (Two launches -- prepare, then an estimate over the prepared
//                              guide records -- would spare the short blocks the halo's divisions, 1.08 records per pixel, and cost every frame a
//                              launch and a second pass over 28 bytes per pixel; the one launch is cheaper exactly when the history is long, which
//                              is the steady state.  1 + levels launches in all.)
//   variance_level_kernel      one level in rtw_denoise's three tilings with its LDS layout; the colour record is (I.xyz, V).  Per tap three more
//                              flops for lum(q), one product for sv.  Before its taps a lane needs g(p), the 3 x 3 prefilter of V_i at distance ONE:
//       GPASS false            in the dense tiling the eight neighbours are in the halo (2 * step >= 2) and come from LDS; in the lattice and direct
//                              tilings they belong to other lattices, and the lane reads their 8 variance words and 8 keys from global memory --
//                              neighbouring pixels of neighbouring lanes, lines its own block or the one beside it has just loaded (L2).
//       GPASS true             variance_prefilter_kernel has written g for every pixel into the workspace (4 more bytes per pixel, one more launch per
//                              level); the lane reads one word.
//                              Both routes run variance_prefilter over the same nine values in the same order: the same bits, whichever tiling.
//                              Which is the default is measured (profiles/variance_experiments.md section 3).
//   The last level (LAST) remodulates and packs as rtw_denoise's does.

#define VE_HALO 3
#define VE_PW (DN_TILE_W + 2 * VE_HALO)
#define VE_PH (DN_TILE_H + 2 * VE_HALO)

struct VarianceBufs {
    const Mu2* __restrict__ moments;        // (mu1, mu2) per pixel (never written)
    float* __restrict__ g;                  // workspace: the prefiltered variance (GPASS)
    int min_history;
    float sigma_lum;                        // <= 0: the luminance term is off and the variance plays no part
    float kn, kd;                           // as DenoiseLevel's
};

// The record of pixel `pixel` as denoise_prepare_kernel makes it; returns the framebuffer's count
__device__ __forceinline__ int variance_record(const DenoiseBufs& b, int pixel, float4& c, float4& gd, uint32_t& key)
{
    const float4 a = b.accum[pixel], g = b.geom[pixel], al = b.albedo[pixel];
    const int cfb = __float_as_int(a.w), cf = __float_as_int(al.w);
    key = (uint32_t)b.ids[pixel] << 2;
    c = make_float4(0.0f, 0.0f, 0.0f, 0.0f); gd = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (cfb == 0 || cf == 0) { key |= DN_EMPTY; return cfb; }
    const float nfb = (float)cfb, nf = (float)cf;
    c = make_float4(a.x / nfb, a.y / nfb, a.z / nfb, 0.0f);
    gd = make_float4(g.x / nf, g.y / nf, g.z / nf, g.w / nf);
    if (!(dn_finite(c.x) && dn_finite(c.y) && dn_finite(c.z))) key |= DN_BAD;
    if (b.flags & rtw::DENOISE_DEMODULATE) { c.x = c.x / (al.x / nf + DN_EPS); c.y = c.y / (al.y / nf + DN_EPS); c.z = c.z / (al.z / nf + DN_EPS); }
    return cfb;
}

__global__ DN_TARGET __launch_bounds__(256) void variance_estimate_kernel(DenoiseBufs b, VarianceBufs v, float4* __restrict__ i0)
{
    __shared__ float4 lg[VE_PW * VE_PH];
    __shared__ Mu2 lm[VE_PW * VE_PH];
    __shared__ uint32_t lk[VE_PW * VE_PH];
    __shared__ int any_short;
    const int t = (int)threadIdx.x, W = b.width, H = b.height, tx = t & (DN_TILE_W - 1), ty = t / DN_TILE_W;
    const int bx = (int)blockIdx.x * DN_TILE_W - VE_HALO, by = (int)blockIdx.y * DN_TILE_H - VE_HALO;
    const int px = bx + VE_HALO + tx, py = by + VE_HALO + ty;
    const bool inside = px < W && py < H;
    const int pixel = inside ? py * W + px : 0;
    if (t == 0) any_short = 0;
    __syncthreads();
    float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), gp = c; uint32_t kp = DN_EMPTY; int n = 0;
    Mu2 mu = { 0.0f, 0.0f };
    if (inside) { n = variance_record(b, pixel, c, gp, kp); mu = v.moments[pixel]; }
    const bool is_short = !(kp & DN_EMPTY) && n < v.min_history;
    if (is_short) any_short = 1;                    // (every writer writes the same word)
    __syncthreads();
    if (any_short) {                                // uniform over the block
        for (int r = t; r < VE_PW * VE_PH; r += 256) {
            const int x = bx + r % VE_PW, y = by + r / VE_PW;
            float4 cq, gq = make_float4(0.0f, 0.0f, 0.0f, 0.0f); uint32_t kq = DN_EMPTY; Mu2 mq = { 0.0f, 0.0f };
            if (x >= 0 && x < W && y >= 0 && y < H) { (void)variance_record(b, y * W + x, cq, gq, kq); mq = v.moments[y * W + x]; }
            lg[r] = gq; lm[r] = mq; lk[r] = kq;
        }
        __syncthreads();
    }
    if (!inside) return;
    float V = 0.0f;
    if (!(kp & DN_EMPTY)) {
        if (!is_short) {
            V = __builtin_fmaxf(mu.y - mu.x * mu.x, 0.0f);
        } else {
            const bool same_shape = (b.flags & rtw::DENOISE_SAME_SHAPE) != 0, use_n = v.kn > 0.0f, use_d = v.kd > 0.0f;
            const float inv_z = use_d ? v.kd / __builtin_fmaxf(__builtin_fabsf(gp.w), 1e-6f) : 0.0f;
            const int cr = (ty + VE_HALO) * VE_PW + tx + VE_HALO;
            float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
            for (int dy = -VE_HALO; dy <= VE_HALO; dy++) {
#pragma unroll
                for (int dx = -VE_HALO; dx <= VE_HALO; dx++) {
                    const int q = cr + dy * VE_PW + dx;
                    const float4 gq = lg[q]; const Mu2 mq = lm[q]; const uint32_t kq = lk[q];
                    const bool take = (kq & (DN_EMPTY | DN_BAD)) == 0 && !(same_shape && ((kq ^ kp) >> 2) != 0);
                    float e = 0.0f;
                    if (use_n) { const float x = gp.x - gq.x, y = gp.y - gq.y, z = gp.z - gq.z; e += (x * x + y * y + z * z) * v.kn; }
                    if (use_d) { const float d = (gp.w - gq.w) * inv_z; e += d * d; }
                    const float w = __builtin_amdgcn_exp2f(-(e * 1.44269504f));       // exp(-e)
                    if (take) { s0 += w; s1 += w * mq.x; s2 += w * mq.y; }
                }
            }
            if (s0 > 0.0f) {
                const float a = s1 / s0;
                V = __builtin_fmaxf(s2 / s0 - a * a, 0.0f) * ((float)v.min_history / (float)n);
            }
        }
    }
    c.w = V;
    i0[pixel] = c; b.guide[pixel] = gp; b.key[pixel] = kp;
}

// g(p): the 3 x 3 prefilter of the variance at distance 1, dy outer, dx inner.  fetch(dx, dy, V, key) hands over V_i and the key of p + (dx, dy);
// a pixel outside the frame comes back with DN_EMPTY.
template <typename Fetch>
__device__ __forceinline__ float variance_prefilter(Fetch&& fetch)
{
    float sk = 0.0f, sv = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            const float k = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f);
            float vq; uint32_t kq;
            fetch(dx, dy, vq, kq);
            if ((kq & (DN_EMPTY | DN_BAD)) == 0) { sk += k; sv += k * vq; }
        }
    }
    return sk > 0.0f ? sv / sk : 0.0f;
}

// ... from global memory (the lattice and direct tilings, and the prefilter pass)
__device__ __forceinline__ float variance_prefilter_global(const float4* __restrict__ in, const uint32_t* __restrict__ key, int px, int py, int W, int H)
{
    return variance_prefilter([&](int dx, int dy, float& vq, uint32_t& kq) {
        const int qx = px + dx, qy = py + dy;
        const bool ok = qx >= 0 && qx < W && qy >= 0 && qy < H;
        const int q = ok ? qy * W + qx : py * W + px;
        vq = in[q].w; kq = ok ? key[q] : DN_EMPTY;
    });
}

__global__ DN_TARGET __launch_bounds__(256) void variance_prefilter_kernel(DenoiseBufs b, const float4* __restrict__ in, float* __restrict__ g)
{
    const int px = (int)blockIdx.x * DN_TILE_W + ((int)threadIdx.x & (DN_TILE_W - 1)), py = (int)blockIdx.y * DN_TILE_H + (int)threadIdx.x / DN_TILE_W;
    if (px >= b.width || py >= b.height) return;
    g[py * b.width + px] = variance_prefilter_global(in, b.key, px, py, b.width, b.height);
}

// The 25 taps of one pixel in rtw_denoise's order with its skip rules, its normal and depth terms and its sums; the colour term is the luminance's,
// scaled by the prefiltered standard deviation g, and sv sums the variance under the squared weights.  cp.w and the fetched cq.w are V_i.
template <typename Fetch>
__device__ __forceinline__ void variance_taps(const DenoiseLevel& L, float sigma_lum, bool same_shape, float4 cp, float4 gp, uint32_t kp, float g, Fetch&& fetch,
                                              float& ox, float& oy, float& oz, float& ov)
{
    const bool pbad = (kp & DN_BAD) != 0;
    const bool use_l = sigma_lum > 0.0f && !pbad, use_n = L.kn > 0.0f, use_d = L.kd > 0.0f;
    const float inv_z = use_d ? L.kd / __builtin_fmaxf(__builtin_fabsf(gp.w), 1e-6f) : 0.0f;
    const float lp = dn_lum(cp.x, cp.y, cp.z), inv_l = use_l ? 1.0f / (sigma_lum * __builtin_sqrtf(g) + 1e-4f) : 0.0f;
    float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f, sv = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const float hx = dx == 0 ? 0.375f : ((dx == 1 || dx == -1) ? 0.25f : 0.0625f), hy = dy == 0 ? 0.375f : ((dy == 1 || dy == -1) ? 0.25f : 0.0625f);
            float4 cq, gq; uint32_t kq;
            fetch(dx, dy, cq, gq, kq);
            const bool take = (kq & (DN_EMPTY | DN_BAD)) == 0 && !(same_shape && ((kq ^ kp) >> 2) != 0);
            float e = 0.0f;
            if (use_l) e += __builtin_fabsf(lp - dn_lum(cq.x, cq.y, cq.z)) * inv_l;
            if (use_n) { const float x = gp.x - gq.x, y = gp.y - gq.y, z = gp.z - gq.z; e += (x * x + y * y + z * z) * L.kn; }
            if (use_d) { const float d = (gp.w - gq.w) * inv_z; e += d * d; }
            const float w = (hx * hy) * __builtin_amdgcn_exp2f(-(e * 1.44269504f));       // exp(-e)
            if (take) { sw += w; sx += w * cq.x; sy += w * cq.y; sz += w * cq.z; sv += (w * w) * cq.w; }
        }
    }
    ov = sw > 0.0f ? sv / (sw * sw) : cp.w;
    if (sw > 0.0f) { ox = sx / sw; oy = sy / sw; oz = sz / sw; }
    else if (!pbad) { ox = cp.x; oy = cp.y; oz = cp.z; }
    else { ox = 0.0f; oy = 0.0f; oz = 0.0f; }
}

template <int TIL, int RX, bool LAST, bool GPASS>
__global__ DN_TARGET __launch_bounds__(256) void variance_level_kernel(DenoiseBufs b, DenoiseLevel L, VarianceBufs v)
{
    __shared__ float thr[LAST ? 256 : 1];
    if (LAST) thr[threadIdx.x] = b.gamma_thr[threadIdx.x];
    const int t = (int)threadIdx.x, W = b.width, H = b.height, step = L.step;
    const bool same_shape = (b.flags & rtw::DENOISE_SAME_SHAPE) != 0, use_g = v.sigma_lum > 0.0f;
    int px, py;                             // this thread's pixel
    float4 cp = make_float4(0.0f, 0.0f, 0.0f, 0.0f), gp = cp; uint32_t kp = DN_EMPTY;
    float ox = 0.0f, oy = 0.0f, oz = 0.0f, ov = 0.0f;
    if (TIL == DN_DIRECT) {
        px = (int)blockIdx.x * DN_TILE_W + (t & (DN_TILE_W - 1)); py = (int)blockIdx.y * DN_TILE_H + t / DN_TILE_W;
        if (LAST) __syncthreads();
        if (px >= W || py >= H) return;
        const int pixel = py * W + px;
        cp = L.in[pixel]; gp = b.guide[pixel]; kp = b.key[pixel];
        if (!(kp & DN_EMPTY)) {
            const float g = !use_g ? 0.0f : (GPASS ? v.g[pixel] : variance_prefilter_global(L.in, b.key, px, py, W, H));
            variance_taps(L, v.sigma_lum, same_shape, cp, gp, kp, g, [&](int dx, int dy, float4& cq, float4& gq, uint32_t& kq) {
                const int qx = px + step * dx, qy = py + step * dy;
                const bool in = qx >= 0 && qx < W && qy >= 0 && qy < H;
                const int q = in ? qy * W + qx : pixel;
                cq = L.in[q]; gq = b.guide[q]; kq = in ? b.key[q] : DN_EMPTY;
            }, ox, oy, oz, ov);
        }
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
        HIP_DYNAMIC_SHARED(float4, vl_lds);                 // [N colour and variance | N guide | N key words]
        float4* lc = vl_lds; float4* lg = vl_lds + N; uint32_t* lk = (uint32_t*)(vl_lds + 2 * N);
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
        if (!(kp & DN_EMPTY)) {
            float g = 0.0f;
            if (use_g) {
                if (GPASS) g = v.g[py * W + px];
                else if (TIL == DN_DENSE) g = variance_prefilter([&](int dx, int dy, float& vq, uint32_t& kq) { const int q = c + dy * PW + dx; vq = lc[q].w; kq = lk[q]; });
                else g = variance_prefilter_global(L.in, b.key, px, py, W, H);
            }
            variance_taps(L, v.sigma_lum, same_shape, cp, gp, kp, g, [&](int dx, int dy, float4& cq, float4& gq, uint32_t& kq) {
                const int q = c + dy * SY + dx * SX;
                cq = lc[q]; gq = lg[q]; kq = lk[q];
            }, ox, oy, oz, ov);
        }
    }
    const int pixel = py * W + px;
    if (!LAST) { L.out[pixel] = make_float4(ox, oy, oz, ov); return; }
    if (!(kp & DN_EMPTY) && (b.flags & rtw::DENOISE_DEMODULATE)) {
        const float4 al = b.albedo[pixel];
        const float nf = (float)__float_as_int(al.w);
        ox = ox * (al.x / nf + DN_EPS); oy = oy * (al.y / nf + DN_EPS); oz = oz * (al.z / nf + DN_EPS);
    }
    b.dst_accum[pixel] = make_float4(ox, oy, oz, __int_as_float(1));
    b.dst_argb[pixel] = pack_pixel(thr, mk(ox, oy, oz));
}
