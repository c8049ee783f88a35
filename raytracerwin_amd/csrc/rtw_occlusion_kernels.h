// rtw_occlusion_kernels.h -- ambient occlusion from the first-hit feature buffers (rtw_render_occlusion; the formula is the header comment of
// include/rtwin.h, its arithmetic rtw_shared.h's occlusion_*).  Included inside rtw_device.hip's anonymous namespace after rtw_query_kernels.h: the
// walk is rtw_group_kernels.h's lane_find_intersection with ANY set, unchanged, as in qtrace_kernel.  Independent rays with data-dependent walks: no
// operand is shared between lanes, so no matrix instruction fits.
//
//   occlusion_kernel   ONE launch for all passes of a call.  Four waves (a GROUP) own an 8 x 8 pixel tile; a block is NT / 256 groups and takes
//                      tiles in a grid-stride loop, so that a tree staged in LDS (STAGE, the query kernels' rule) is paid for once per block and not
//                      once per tile.  Per tile:
//     prologue         wave 0 of the group, a lane per pixel: the pixel's 40 feature bytes -> state (EMPTY / OPEN / CAST), unit normal n and ray
//                      origin O (occlusion_origin), put in LDS for the group's other waves; the lane keeps the pixel's accumulator entry in
//                      registers from here to the end (ONE read and ONE write of it per call).  One ballot and an LDS flag per group: a block none
//                      of whose tiles holds a casting pixel (sky, empty rows of another rank) adds a = 1 per pass to its OPEN pixels and goes on to
//                      its next tiles before anything is staged or walked.
//     rays             a pass of a tile is 64 x samples rays, in `samples` chunks of 64; wave w of the group takes chunks w, w + 4, ...  Ray
//                      r = chunk * 64 + lane is, BYSAMPLE false (lane per pixel): sample `chunk` of pixel `lane` -- O and n stay in the lane's
//                      registers for the whole tile, only the 12-byte table entry changes per ray, and a wave's 64 rays start from 64 neighbouring
//                      surface points; BYSAMPLE true (lane per sample): sample r % samples of pixel r / samples -- a wave holds 64 / samples pixels
//                      with all their samples, origins shared exactly, directions spread over the hemisphere; O and n come from LDS per ray.
//                      The table entry of the wave's next chunk is requested before the walk of the current one starts (every entry is an HBM miss).
//                      Rays are `radius` long: most lanes leave at a shape's slab test and the walk's wave-uniform ballots skip the shape.
//     reduction        the chunk's occlusion bits are ONE ballot, stored as 64 bits per chunk; a ray's weight c_s goes to cw[r].  After a barrier
//                      the pixel's lane of wave 0 adds t_s and c_s for s = 0, 1, ... in order, divides, and adds a to its accumulator registers.
//                      No atomic and no order of arrival anywhere: a ballot and plain stores to slots of one's own.  A second barrier frees the
//                      slots for the next pass.  After the last pass: the accumulator's write and ARGB through the gamma thresholds held in LDS.
//   LDS (words): [CAP * NT candidate lists | per group: 8 x 64 pixel words (O, n, state, pad), 64 x 2 ballot words, samples x 64 weights | staged
//   records].  Pixel words and weights are read at lane-consecutive addresses (BYSAMPLE false) or as 64 / samples broadcasts (true): no bank conflicts.

#define OC_TILE 8
#define OC_PIX_WORDS 512
#define OC_OCC_WORDS 128
__host__ __device__ constexpr int oc_group_words(int samples) { return OC_PIX_WORDS + OC_OCC_WORDS + samples * 64; }

struct OcclusionBufs {
    const float4* __restrict__ geom;        // (sum normal.xyz, sum depth)
    const float4* __restrict__ albedo;      // (sum rgb, int count)
    const unsigned long long* __restrict__ ids;     // shape in the low word
    float4* __restrict__ accum;             // (sum.xyz, int count)
    uint32_t* __restrict__ argb;
    const float* __restrict__ gamma_thr;
    RtwCamera cam;
    int width, height, tiles_x, n_tiles;
    float radius, bias;
    int samples, cosine;
    int first_pass, n_passes;
    uint32_t seed;
};

__device__ __forceinline__ f3 oc_table_entry(const RtwSceneDev* __restrict__ sc, const OcclusionBufs& b, uint32_t pixel, int pass, int s)
{
    const size_t i = (size_t)occlusion_table_index(b.seed, pixel, (uint32_t)pass, (uint32_t)s) * 3;
    const float* e = sc->unit_table;
    return mk(gld1(e, i), gld1(e, i + 1), gld1(e, i + 2));
}

template <bool AN, int NT, int CAP, int STAGE, bool BYSAMPLE>
__global__ __launch_bounds__(NT) void occlusion_kernel(const RtwSceneDev* __restrict__ sc, OcclusionBufs b, int staged_shape, int staged_top)
{
    static_assert(NT % 256 == 0, "four waves to a tile");
    constexpr int G = NT / 256;
    HIP_DYNAMIC_SHARED(uint32_t, gt_dyn);               // [CAP * NT candidate words | G groups' words | staged records]
    __shared__ float thr[256];
    __shared__ int casts[G];
    uint32_t* cand = gt_dyn;
    const int tid = (int)threadIdx.x, lane = lane_id(), g = tid >> 8, w = (tid >> 6) & 3;
    const int S = b.samples, W = b.width, H = b.height;
    uint32_t* gw = gt_dyn + CAP * NT + g * oc_group_words(S);
    uint32_t* pixw = gw; uint32_t* occ = gw + OC_PIX_WORDS; uint32_t* cw = gw + OC_PIX_WORDS + OC_OCC_WORDS;
    if (tid < 256) thr[tid] = b.gamma_thr[tid];
    const float4* lnodes = nullptr; int ltop = 0;
    bool staged_done = false;
    Counters ct = { 0, 0, 0, 0, 0, 0 };
    for (int t0 = (int)blockIdx.x * G; t0 < b.n_tiles; t0 += (int)gridDim.x * G) {          // block-uniform
        const int tile = t0 + g;
        const int tx = (tile % b.tiles_x) * OC_TILE, ty = (tile / b.tiles_x) * OC_TILE;      // (a group past the last tile: every pixel outside the frame)
        // ---- prologue: wave 0 of the group, a lane per pixel ----
        int fstate = RTW_OC_EMPTY, fpixel = 0; float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (w == 0) {
            const int px = tx + (lane & 7), py = ty + (lane >> 3);
            f3 O = mk(0.0f, 0.0f, 0.0f), n = mk(0.0f, 0.0f, 0.0f);
            if (tile < b.n_tiles && px < W && py < H) {
                fpixel = py * W + px;
                const int cf = __float_as_int(b.albedo[fpixel].w);
                if (cf != 0) {
                    const float4 gm = b.geom[fpixel];
                    fstate = occlusion_origin(b.cam, px, py, W, H, gm.x, gm.y, gm.z, gm.w, cf, (int)(uint32_t)b.ids[fpixel], b.bias, O, n);
                    acc = b.accum[fpixel];
                }
            }
            lstu(pixw, lane, __float_as_uint(O.x)); lstu(pixw, 64 + lane, __float_as_uint(O.y)); lstu(pixw, 128 + lane, __float_as_uint(O.z));
            lstu(pixw, 192 + lane, __float_as_uint(n.x)); lstu(pixw, 256 + lane, __float_as_uint(n.y)); lstu(pixw, 320 + lane, __float_as_uint(n.z));
            lstu(pixw, 384 + lane, (uint32_t)fstate);
            const bool any = __ballot(fstate == RTW_OC_CAST) != 0ull;
            if (lane == 0) casts[g] = any ? 1 : 0;
        }
        __syncthreads();
        bool block_casts = false;
#pragma unroll
        for (int k = 0; k < G; k++) block_casts = block_casts || casts[k] != 0;
        if (!block_casts) {                             // (whole block) nothing to walk: a = 1 per pass, added one by one as the passes would
            if (w == 0 && fstate != RTW_OC_EMPTY) {
                int cnt = __float_as_int(acc.w);
                for (int k = 0; k < b.n_passes; k++) { acc.x += 1.0f; acc.y += 1.0f; acc.z += 1.0f; cnt++; }
                const float nf = (float)cnt;
                b.accum[fpixel] = make_float4(acc.x, acc.y, acc.z, __int_as_float(cnt));
                b.argb[fpixel] = pack_pixel(thr, mk(acc.x / nf, acc.y / nf, acc.z / nf));
            }
            __syncthreads();                            // the next tiles' prologue rewrites the group words and the flags
            continue;
        }
        if (STAGE && !staged_done) {                    // (whole block) the first tile with work pays for the tree
            float4* dst = reinterpret_cast<float4*>(gt_dyn + CAP * NT + G * oc_group_words(S));
            const float4* src4 = reinterpret_cast<const float4*>(sc->shapes[staged_shape].tnodes);
            for (int i = tid; i < staged_top * 2; i += NT) dst[i] = gld4(src4, (size_t)i);
            lnodes = dst; ltop = staged_top;
            staged_done = true;
            __syncthreads();
        }
        // ---- the lane's pixel, BYSAMPLE false: its own for the whole tile ----
        int p = lane, st = 0; f3 O = mk(0.0f, 0.0f, 0.0f), n = mk(0.0f, 0.0f, 0.0f);
        auto load_pixel = [&](int q) {
            O = mk(__uint_as_float(lldu(pixw, q)), __uint_as_float(lldu(pixw, 64 + q)), __uint_as_float(lldu(pixw, 128 + q)));
            n = mk(__uint_as_float(lldu(pixw, 192 + q)), __uint_as_float(lldu(pixw, 256 + q)), __uint_as_float(lldu(pixw, 320 + q)));
            st = (int)lldu(pixw, 384 + q);
        };
        // pixel index of the tile's pixel q for the random stream (a pixel outside the frame casts nothing: any value will do)
        auto pixel_of = [&](int q) { return (uint32_t)((ty + (q >> 3)) * W + tx + (q & 7)); };
        if (!BYSAMPLE) load_pixel(lane);
        const bool group_casts = casts[g] != 0;         // (a group without a casting pixel walks nothing, but keeps the block's barriers)
        int cnt = __float_as_int(acc.w);
        for (int k = 0; k < b.n_passes; k++) {
            const int pass = b.first_pass + k;
            if (group_casts) {
                int s = w;
                if (BYSAMPLE) { const int r = w * 64 + lane; p = r / S; s = r - p * S; }
                f3 vnext = mk(0.0f, 0.0f, 1.0f);
                if (w < S) vnext = oc_table_entry(sc, b, pixel_of(p), pass, s);
                for (int c = w; c < S; c += 4) {        // wave-uniform
                    if (BYSAMPLE) load_pixel(p);
                    const f3 v = vnext;
                    const int r = c * 64 + lane;
                    if (c + 4 < S) {                    // the next chunk's entry, requested ahead of this chunk's walk
                        if (BYSAMPLE) { const int rn = (c + 4) * 64 + lane; p = rn / S; s = rn - p * S; } else s = c + 4;
                        vnext = oc_table_entry(sc, b, pixel_of(p), pass, s);
                    }
                    const bool have = st == RTW_OC_CAST;
                    const f3 d = occlusion_direction(v, n);
                    const float cs = occlusion_weight(n, d, b.cosine != 0);
                    Ray ray; ray.o = mk(0, 0, 0); ray.d = mk(0, 0, 1); ray.dist = 0.0f;
                    if (have) { ray.o = O; ray.d = d; ray.dist = b.radius; }
                    int hs = -1, hslot = -1, cshape = -1, cslot = -1; f3 pos = mk(0, 0, 0), cpos = mk(0, 0, 0); float seg = ray.dist, cdist = 0.0f;
                    lane_find_intersection<false, AN, NT, CAP, (STAGE == 2), true>(sc, cand, lnodes, ltop, STAGE ? staged_shape : -1, ray, have, 0, hs, hslot, pos, seg, cshape, cslot, cpos, cdist, ct);
                    const unsigned long long bits = __ballot(have && hs >= 0);
                    if (lane == 0) { lstu(occ, 2 * c, (uint32_t)bits); lstu(occ, 2 * c + 1, (uint32_t)(bits >> 32)); }
                    lstu(cw, r, __float_as_uint(cs));
                }
            }
            __syncthreads();
            if (w == 0 && fstate != RTW_OC_EMPTY) {     // the pixel's lane: t_s and c_s in the order of s
                float a = 1.0f;
                if (fstate == RTW_OC_CAST) {
                    float A = 0.0f, Wt = 0.0f;
                    for (int s = 0; s < S; s++) {
                        const int r = BYSAMPLE ? lane * S + s : s * 64 + lane;
                        const bool hit = ((lldu(occ, r >> 5) >> (r & 31)) & 1u) != 0u;
                        const float cs = __uint_as_float(lldu(cw, r));
                        A += hit ? 0.0f : cs; Wt += cs;
                    }
                    a = Wt > 0.0f ? A / Wt : 1.0f;
                }
                acc.x += a; acc.y += a; acc.z += a; cnt++;
            }
            __syncthreads();
        }
        if (w == 0 && fstate != RTW_OC_EMPTY) {
            const float nf = (float)cnt;
            b.accum[fpixel] = make_float4(acc.x, acc.y, acc.z, __int_as_float(cnt));
            b.argb[fpixel] = pack_pixel(thr, mk(acc.x / nf, acc.y / nf, acc.z / nf));
        }
    }
}
