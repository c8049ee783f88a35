// rtw_reproject_kernels.h -- temporal reprojection: the history a pixel's first hit had in the previous frame, fetched through the previous camera,
// kept where it shows the same surface and blended with the new sample (rtw_reproject; the formula is the header comment of include/rtwin.h, its
// projection arithmetic is rtw_shared.h's reproject_*).  Included inside rtw_device.hip's anonymous namespace after rtw_denoise_kernels.h, whose
// DN_TARGET (no packed fp32 instructions) and dn_finite it uses, with pack_pixel.  A data-dependent gather with a validity test per tap: no operand is
// shared between pixels, so no matrix instruction fits, and the kernel is about moving records.
//
//   reproject_kernel<STAGED>   ONE launch, 256 threads, a lane per output pixel, a block owns a 32 x 8 tile (a wave is 2 rows of 32).  A lane reads its
//                              own pixel's four words (56 bytes), makes its record, projects it (steps 1 to 3) and hands the tap routine
//                              (reproject_taps) the records of its up to four history pixels; then the blend, the remodulation, the pack through the
//                              gamma thresholds held in LDS, and 20 bytes written.  Both variants build a history pixel's record with the SAME function
//                              (rp_record) and run the SAME tap routine, so a pixel's bits do not depend on which ran (-ffp-contract=off).
//     direct (STAGED false)    every tap reads its pixel's four words from global memory (L2): 56 bytes and five divisions per tap.  Neighbouring lanes
//                              share cache lines; nothing is staged.
//     staged (STAGED true)     the block reduces the bounding box of its lanes' in-frame taps of non-zero weight (four __shfl_xor butterflies per wave,
//                              then the four waves through 16 words of LDS).  A box of at most RP_BOX_MAX pixels is loaded once -- coalesced 16-byte
//                              loads, row by row -- turned into RECORDS and kept in LDS; the taps read LDS.  A larger box (strong zoom, roll, a depth
//                              edge through the tile) sends that block down the direct path: a per-block decision, uniform over its waves.
//   A record is what a tap needs and nothing else: colour = (I.xyz, history length as int bits), geom = (n.xyz, z), key = shape << 2 | RP_BAD | RP_EMPTY,
//   36 bytes.  The divisions by the two counts and the demodulation are done when the record is made, so the staged variant does them once per history
//   pixel instead of once per tap, and needs no albedo array in LDS: 640 records are 22.5 KiB, six blocks to a CU.
//   LDS layout: three arrays of RP_BOX_MAX entries, colour float4 | geom float4 | key uint32, record (i, j) of the PW x PH box at j * PW + i with the
//   box's own PW (no padding).  Bank conflicts: a 16-byte LDS read is served a quarter wave at a time, and its 16 lanes are neighbours in one row of
//   the tile.  Unmoved or panned, they read 16 neighbouring records = 256 contiguous bytes, every bank once, for any PW.  Under a dolly or a small
//   rotation neighbouring lanes' x0 differ by 0, 1 or 2: equal addresses are one broadcast read, and the 16 records span at most 32 entries, two
//   reads per bank at the worst -- for any PW again, since the lanes of a quarter wave share their row.  Nothing is padded.  The 4-byte key reads
//   come from at most 2 x 64 neighbouring words.
//   The tail packs ARGB through the gamma thresholds held in LDS, as the denoiser's last level does.
//   reproject_moments_kernel<STAGED>   rtw_reproject_moments: the same body (reproject_body<STAGED, MOMENTS>) with the luminance moments riding along.  A
//                              history pixel's record carries its (mu1, mu2) as two more floats -- 44 bytes -- and reproject_taps sums them under the
//                              colour's weights and validity: the projection, the taps and the tests run once.  The staged box shrinks to
//                              RP_BOX_MAX_M = 576 records (24.75 KiB, a tile plus a border of 4 x 4 or 8 x 2 pixels), which keeps six blocks to a CU; a
//                              larger box takes the direct path as before, so the bits do not depend on the limit.  The tail blends (l, l * l) of the
//                              current sample into the moments by the colour's own cases and writes 8 more bytes.

#define RP_EMPTY 1u         // key bit: one of the pixel's two counts is 0
#define RP_BAD 2u           // key bit: a channel of the pixel's colour is not finite
#define RP_EPS 1e-3f
#define RP_TILE_W 32
#define RP_TILE_H 8
#define RP_BOX_MAX 640      // records a block stages at most: 2.5 tiles, e.g. the tile plus a border of 6 x 4 pixels, or a zoom of 1.5
#define RP_BOX_MAX_M 576    // ... with moments (44-byte records): 2.25 tiles, six blocks to a CU as without

struct ReprojectFrame {     // a framebuffer and its feature buffers
    const float4* __restrict__ accum;       // (sum.xyz, int count)
    const float4* __restrict__ geom;        // (sum normal.xyz, sum depth)
    const float4* __restrict__ albedo;      // (sum rgb, int count)
    const unsigned long long* __restrict__ ids;     // shape in the low word
};
struct ReprojectBufs {
    ReprojectFrame cur, hist;
    float4* __restrict__ dst_accum;
    uint32_t* __restrict__ dst_argb;
    const float* __restrict__ gamma_thr;
    RtwCamera cam_cur, cam_prev;
    int width, height, max_history;
    float depth_tolerance, normal_cos;
    uint32_t flags;                         // REPROJECT_DEMODULATE
};
struct RpRecord { float4 c, g; uint32_t key; };
struct __attribute__((aligned(8))) Mu2 { float x, y; };     // a pixel's luminance moments (mu1, mu2)
struct ReprojectMoments {   // rtw_reproject_moments: the history's moments, the destination's, and moments_history
    const Mu2* __restrict__ hist;
    Mu2* __restrict__ dst;
    int history;
};
struct RpRecordM : RpRecord { Mu2 m; };     // a history record with its moments
template <bool MOMENTS> struct RpRec { typedef RpRecord type; };
template <> struct RpRec<true> { typedef RpRecordM type; };
__device__ __forceinline__ void rp_moments_load(RpRecord&, const Mu2*, int) {}
__device__ __forceinline__ void rp_moments_load(RpRecordM& q, const Mu2* a, int i) { q.m = a[i]; }
__device__ __forceinline__ void rp_moments_tap(const RpRecord&, float, Mu2&) {}
__device__ __forceinline__ void rp_moments_tap(const RpRecordM& q, float w, Mu2& sm) { sm.x += w * q.m.x; sm.y += w * q.m.y; }
__device__ __forceinline__ float dn_lum(float x, float y, float z) { return (0.2126f * x + 0.7152f * y) + 0.0722f * z; }

// The record of pixel `pixel` of frame f; mod = A + EPS per channel (what a demodulated colour was divided by), zeros for an empty pixel
__device__ __forceinline__ RpRecord rp_record(const ReprojectFrame& f, int pixel, bool demodulate, f3& mod)
{
    const float4 a = f.accum[pixel], g = f.geom[pixel], al = f.albedo[pixel];
    const int cfb = __float_as_int(a.w), cf = __float_as_int(al.w);
    RpRecord r;
    r.key = (uint32_t)f.ids[pixel] << 2;
    r.c = make_float4(0.0f, 0.0f, 0.0f, a.w); r.g = make_float4(0.0f, 0.0f, 0.0f, 0.0f); mod = mk(0.0f, 0.0f, 0.0f);
    if (cfb == 0 || cf == 0) { r.key |= RP_EMPTY; return r; }
    const float nfb = (float)cfb, nf = (float)cf;
    r.c.x = a.x / nfb; r.c.y = a.y / nfb; r.c.z = a.z / nfb;
    r.g = make_float4(g.x / nf, g.y / nf, g.z / nf, g.w / nf);
    if (!(dn_finite(r.c.x) && dn_finite(r.c.y) && dn_finite(r.c.z))) r.key |= RP_BAD;
    mod = mk(al.x / nf + RP_EPS, al.y / nf + RP_EPS, al.z / nf + RP_EPS);
    if (demodulate) { r.c.x = r.c.x / mod.x; r.c.y = r.c.y / mod.y; r.c.z = r.c.z / mod.z; }
    return r;
}

// The four taps of one pixel in the stated order.  fetch(qx, qy, record) hands over the record of the history pixel (qx, qy), and is only asked for
// pixels inside the frame whose weight is not 0.  sw = the valid taps' weight, s = their weighted colours, nh = the smallest history length among them;
// sm = their weighted moments when the records (Rec) carry any.
template <typename Rec, typename Fetch>
__device__ __forceinline__ void reproject_taps(const ReprojectBufs& b, int x0, int y0, float tx, float ty, const RpRecord& p, float z_exp, Fetch&& fetch,
                                               float& sw, f3& s, int& nh, Mu2& sm)
{
    const bool use_d = b.depth_tolerance > 0.0f, use_n = (p.key >> 2) != 0x3fffffffu && b.normal_cos > -1.0f;      // (a miss has no normal to compare)
    const float zt = b.depth_tolerance * z_exp;
    const float wx[2] = { 1.0f - tx, tx }, wy[2] = { 1.0f - ty, ty };
    sw = 0.0f; s = mk(0.0f, 0.0f, 0.0f); nh = INT_MAX; sm.x = 0.0f; sm.y = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
        const float w = wx[k & 1] * wy[k >> 1];
        if (w == 0.0f || qx < 0 || qx >= b.width || qy < 0 || qy >= b.height) continue;
        Rec q;
        fetch(qx, qy, q);
        bool valid = (q.key & (RP_EMPTY | RP_BAD)) == 0 && ((q.key ^ p.key) >> 2) == 0;
        if (use_d) valid = valid && __builtin_fabsf(q.g.w - z_exp) <= zt;
        if (use_n) valid = valid && dot(mk(p.g.x, p.g.y, p.g.z), mk(q.g.x, q.g.y, q.g.z)) >= b.normal_cos;
        if (valid) {
            const int n = __float_as_int(q.c.w);
            sw += w; s.x += w * q.c.x; s.y += w * q.c.y; s.z += w * q.c.z;
            nh = n < nh ? n : nh;
            rp_moments_tap(q, w, sm);
        }
    }
}

template <bool STAGED, bool MOMENTS>
__device__ __forceinline__ DN_TARGET void reproject_body(const ReprojectBufs& b, const ReprojectMoments& m)
{
    typedef typename RpRec<MOMENTS>::type Rec;
    constexpr int BOX = MOMENTS ? RP_BOX_MAX_M : RP_BOX_MAX;
    __shared__ float thr[256];
    __shared__ int box[STAGED ? 16 : 1];            // per wave: min x, min y, max x, max y of its lanes' taps
    const int t = (int)threadIdx.x, W = b.width, H = b.height;
    thr[t] = b.gamma_thr[t];
    const int px = (int)blockIdx.x * RP_TILE_W + (t & (RP_TILE_W - 1)), py = (int)blockIdx.y * RP_TILE_H + t / RP_TILE_W;
    const bool inside = px < W && py < H, demodulate = (b.flags & rtw::REPROJECT_DEMODULATE) != 0;
    const int pixel = inside ? py * W + px : 0;
    RpRecord p; f3 mod = mk(0.0f, 0.0f, 0.0f);
    p.key = RP_EMPTY;
    if (inside) p = rp_record(b.cur, pixel, demodulate, mod);
    bool taps = false;                              // some tap of this lane may lie in the frame
    int x0 = 0, y0 = 0; float tx = 0.0f, ty = 0.0f, z_exp = 0.0f;
    if (!(p.key & RP_EMPTY)) {
        float fx, fy;
        taps = reproject_project(b.cam_prev, reproject_point(b.cam_cur, px, py, W, H, p.g.w), W, H, fx, fy, z_exp) && reproject_corner(fx, fy, W, H, x0, y0, tx, ty);
    }
    bool staged = false;
    int bx = 0, by = 0, PW = 0;
    float4 *lc = nullptr, *lg = nullptr; uint32_t* lk = nullptr; Mu2* lm = nullptr;
    if (STAGED) {
        HIP_DYNAMIC_SHARED(float4, rp_lds);         // [BOX colour | BOX geom | BOX key words | with moments: BOX moments]
        lc = rp_lds; lg = rp_lds + BOX; lk = (uint32_t*)(rp_lds + 2 * BOX);
        if (MOMENTS) lm = (Mu2*)(lk + BOX);
        // this lane's taps of non-zero weight, clipped to the frame (a lane without any takes no part: an inverted interval)
        int lo_x = x0 < 0 ? 0 : x0, hi_x = x0 + (tx > 0.0f ? 1 : 0), lo_y = y0 < 0 ? 0 : y0, hi_y = y0 + (ty > 0.0f ? 1 : 0);
        hi_x = hi_x > W - 1 ? W - 1 : hi_x; hi_y = hi_y > H - 1 ? H - 1 : hi_y;
        if (!taps || lo_x > hi_x || lo_y > hi_y) { lo_x = lo_y = INT_MAX; hi_x = hi_y = INT_MIN; }
        for (int o = 32; o > 0; o >>= 1) {
            const int ax = __shfl_xor(lo_x, o), ay = __shfl_xor(lo_y, o), cx = __shfl_xor(hi_x, o), cy = __shfl_xor(hi_y, o);
            lo_x = ax < lo_x ? ax : lo_x; lo_y = ay < lo_y ? ay : lo_y; hi_x = cx > hi_x ? cx : hi_x; hi_y = cy > hi_y ? cy : hi_y;
        }
        if ((t & 63) == 0) { int* w = box + 4 * (t >> 6); w[0] = lo_x; w[1] = lo_y; w[2] = hi_x; w[3] = hi_y; }
        __syncthreads();
        for (int w = 0; w < 16; w += 4) {
            lo_x = box[w] < lo_x ? box[w] : lo_x; lo_y = box[w + 1] < lo_y ? box[w + 1] : lo_y;
            hi_x = box[w + 2] > hi_x ? box[w + 2] : hi_x; hi_y = box[w + 3] > hi_y ? box[w + 3] : hi_y;
        }
        // (an empty box -- no lane has a tap -- is "staged" with nothing to load)
        const int PH = hi_y >= lo_y ? hi_y - lo_y + 1 : 0;
        PW = hi_x >= lo_x ? hi_x - lo_x + 1 : 0; bx = lo_x; by = lo_y;
        const long long n = (long long)PW * PH;
        staged = n <= BOX;
        if (staged) {
            for (int r = t; r < (int)n; r += 256) {
                f3 unused;
                const int hp = (by + r / PW) * W + bx + r % PW;
                const RpRecord q = rp_record(b.hist, hp, demodulate, unused);
                lc[r] = q.c; lg[r] = q.g; lk[r] = q.key;
                if (MOMENTS) lm[r] = m.hist[hp];
            }
            __syncthreads();
        }
    } else {
        __syncthreads();
    }
    if (!inside) return;
    float sw = 0.0f; f3 s = mk(0.0f, 0.0f, 0.0f); int nh = INT_MAX; Mu2 sm = { 0.0f, 0.0f };
    if (taps) {
        if (STAGED && staged)
            reproject_taps<Rec>(b, x0, y0, tx, ty, p, z_exp, [&](int qx, int qy, Rec& q) {
                const int r = (qy - by) * PW + (qx - bx);
                q.c = lc[r]; q.g = lg[r]; q.key = lk[r]; rp_moments_load(q, lm, r);
            }, sw, s, nh, sm);
        else
            reproject_taps<Rec>(b, x0, y0, tx, ty, p, z_exp, [&](int qx, int qy, Rec& q) {
                f3 unused; static_cast<RpRecord&>(q) = rp_record(b.hist, qy * W + qx, demodulate, unused); rp_moments_load(q, m.hist, qy * W + qx);
            }, sw, s, nh, sm);
    }
    const bool pbad = (p.key & RP_BAD) != 0;
    if (MOMENTS) {                                  // (l, l * l) blended by the colour's cases, moments_history in max_history's place
        Mu2 mu = { 0.0f, 0.0f };
        if (!(p.key & RP_EMPTY)) {
            const float l = dn_lum(p.c.x, p.c.y, p.c.z), l2 = l * l;
            if (sw > 0.0f) {
                mu.x = sm.x / sw; mu.y = sm.y / sw;
                if (!pbad) {
                    const float nm = (float)(nh >= m.history ? m.history : nh + 1);
                    mu.x = mu.x + (l - mu.x) / nm; mu.y = mu.y + (l2 - mu.y) / nm;
                }
            } else if (!pbad) { mu.x = l; mu.y = l2; }
        }
        m.dst[pixel] = mu;
    }
    f3 I = mk(0.0f, 0.0f, 0.0f); int N = 0;
    if (p.key & RP_EMPTY) {
    } else if (sw > 0.0f) {
        const f3 ih = mk(s.x / sw, s.y / sw, s.z / sw);
        if (!pbad) {
            N = nh >= b.max_history ? b.max_history : nh + 1;
            const float nf = (float)N;
            I = mk(ih.x + (p.c.x - ih.x) / nf, ih.y + (p.c.y - ih.y) / nf, ih.z + (p.c.z - ih.z) / nf);
        } else { I = ih; N = nh; }
    } else if (!pbad) { I = mk(p.c.x, p.c.y, p.c.z); N = 1; }
    if (N > 0 && demodulate) I = mk(I.x * mod.x, I.y * mod.y, I.z * mod.z);
    const float nf = (float)N;
    const float4 out = N > 0 ? make_float4(I.x * nf, I.y * nf, I.z * nf, __int_as_float(N)) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    b.dst_accum[pixel] = out;
    b.dst_argb[pixel] = N > 0 ? pack_pixel(thr, mk(out.x / nf, out.y / nf, out.z / nf)) : pack_pixel(thr, mk(0.0f, 0.0f, 0.0f));
}

template <bool STAGED>
__global__ DN_TARGET __launch_bounds__(256) void reproject_kernel(ReprojectBufs b) { reproject_body<STAGED, false>(b, ReprojectMoments()); }
template <bool STAGED>
__global__ DN_TARGET __launch_bounds__(256) void reproject_moments_kernel(ReprojectBufs b, ReprojectMoments m) { reproject_body<STAGED, true>(b, m); }
