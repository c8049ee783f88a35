// rtw_lighting_kernels.h -- direct lighting from the first-hit feature buffers: point and directional lights with shadow rays (rtw_render_lighting; the
// formula is the header comment of include/rtwin.h, its arithmetic rtw_shared.h's occlusion_origin and lighting_*).  Included inside rtw_device.hip's
// anonymous namespace after rtw_occlusion_kernels.h: the walk is rtw_group_kernels.h's lane_find_intersection with ANY set, unchanged, as in
// qtrace_kernel.  Independent rays with data-dependent walks: no operand is shared between lanes, so no matrix instruction fits.
//
//   lighting_kernel    ONE launch for all passes of a call.  A block of NT threads owns NT / 4 pixels at a time -- G = NT / 256 tiles of 8 x 8 -- and
//                      takes such tile groups in a grid-stride loop, so that a tree staged in LDS (STAGE, the query kernels' rule) is paid for once per
//                      block.  The unit of work is a JOB: (pixel, light j, sample s), job number m = j * samples + s < 64 within its pixel and pass.
//                      About half of all jobs are dead before any walk -- the light is behind the pixel's surface -- which is what the split is for.
//     prologue         the block's first G waves, a lane per pixel (the pixel's OWNER): the 40 feature bytes -> state (EMPTY / OPEN / CAST), unit
//                      normal n and ray origin O (occlusion_origin), put in LDS with the pixel's index for every wave of the block; the owner keeps the
//                      accumulator entry and the albedo factor in registers to the end (ONE read and ONE write of the entry per call).  The light
//                      records go from the launch's arguments to LDS once per block.  A block none of whose tiles holds a casting pixel adds the OPEN
//                      pixels' value per pass and goes on to its next tiles before anything is staged or walked (the occlusion kernel's early out).
//     jobs             a pass is n_lights x samples x G CHUNKS of 64 jobs: chunk c = job m = c / G of the 64 pixels of tile c % G, so the light and the
//                      sample are wave-uniform and the pixel words are read at lane-consecutive LDS addresses.  Wave w of the block takes the chunks
//                      w, w + NT / 64, ...  Every job runs steps 2 to 5 (the table entry for a light with a radius, the ray, the cosine: lt_job).
//       COMPACT false  positional: the lanes of the chunk whose job survived the cull walk at once, the others sit the walk out.
//       COMPACT true   compacted: the survivors' ids (pixel slot << 6 | m) go to a dense LDS queue -- one ballot, a popcount prefix and ONE atomic add
//                      on an LDS counter per chunk -- in ROUNDS of up to LT_ROUND chunks per wave (the queue holds LT_ROUND x NT ids).  After a barrier
//                      wave w takes the queue's entries [64 w, 64 w + 64), [64 (w + NT / 64), ...): 64 live rays a walk, or the queue's tail.  A
//                      queue entry is 4 bytes, not the ray: the lane that takes it runs lt_job again (O and n from LDS at the entry's pixel slot,
//                      the table entry from the cache the first look filled).  Culled jobs never occupy a lane of a walk.
//     results          an occluded job sets bit m of its pixel's 64-bit mask: an LDS OR on one of the two halves (lds_or).  The word is an integer
//                      that does not depend on who came first.  After a barrier the owner folds steps 6 to 8 in job order -- c * att of a job is
//                      recomputed, not stored -- adds e to its accumulator registers and clears its mask.  No float atomic and nothing that depends on
//                      the order of arrival anywhere.  After the last pass: the accumulator's write and ARGB through the gamma thresholds held in LDS.
//   LDS (words): [CAP * NT candidate lists | 8 x NT / 4 pixel words (O, n, state, pixel) | 2 x NT / 4 mask words | LT_ROUND x NT queue (COMPACT) |
//   staged records] + static: 256 thresholds, 72 light words, G flags, two queue counters (one filling or draining, the other being cleared).

#define LT_TILE 8
#define LT_ROUND 4
__host__ __device__ constexpr int lt_block_words(int nt, bool compact) { return (nt / 4) * 10 + (compact ? LT_ROUND * nt : 0); }

struct LightingBufs {
    const float4* __restrict__ geom;        // (sum normal.xyz, sum depth)
    const float4* __restrict__ albedo;      // (sum rgb, int count)
    const unsigned long long* __restrict__ ids;     // shape in the low word
    float4* __restrict__ accum;             // (sum.xyz, int count)
    uint32_t* __restrict__ argb;
    const float* __restrict__ gamma_thr;
    RtwCamera cam;
    int width, height, tiles_x, n_tiles;
    float bias;
    int samples, n_lights, use_albedo;
    int first_pass, n_passes;
    uint32_t seed;
    RtwLight lights[RTW_LT_MAX];
};

// steps 2 to 5 of job (light j, sample s) of pass `pass` of the pixel `pixel` whose rays start at O under the normal n; lw = the light records in LDS
__device__ __forceinline__ bool lt_job(const RtwSceneDev* __restrict__ sc, const uint32_t* lw, uint32_t seed, uint32_t pixel, int pass, int j, int s, f3 O, f3 n, f3& d, float& dist, float& t)
{
    RtwLight L;
    L.type = (int32_t)lldu(lw, j * 9); L.flags = lldu(lw, j * 9 + 1);
#pragma unroll
    for (int k = 0; k < 3; k++) { L.v[k] = __uint_as_float(lldu(lw, j * 9 + 2 + k)); L.color[k] = 0.0f; }
    L.radius = __uint_as_float(lldu(lw, j * 9 + 8));
    f3 u = mk(0.0f, 0.0f, 0.0f);
    if (L.radius != 0.0f) {
        const size_t i = (size_t)lighting_table_index(seed, pixel, (uint32_t)pass, (uint32_t)s, (uint32_t)j) * 3;
        const float* e = sc->unit_table;
        u = mk(gld1(e, i), gld1(e, i + 1), gld1(e, i + 2));
    }
    return lighting_ray(L, u, O, n, d, dist, t);
}

template <bool AN, int NT, int CAP, int STAGE, bool COMPACT>
__global__ __launch_bounds__(NT) void lighting_kernel(const RtwSceneDev* __restrict__ sc, LightingBufs b, int staged_shape, int staged_top)
{
    static_assert(NT % 256 == 0, "a tile to every four waves");
    constexpr int G = NT / 256, NW = NT / 64, NP = NT / 4;
    HIP_DYNAMIC_SHARED(uint32_t, gt_dyn);               // [CAP * NT candidate words | pixel words | masks | queue | staged records]
    __shared__ float thr[256];
    __shared__ uint32_t lw[RTW_LT_MAX * 9];
    __shared__ int casts[G];
    __shared__ uint32_t qn[2];
    uint32_t* cand = gt_dyn;
    uint32_t* pixw = gt_dyn + CAP * NT; uint32_t* mask = pixw + 8 * NP; uint32_t* queue = mask + 2 * NP;
    const int tid = (int)threadIdx.x, lane = lane_id(), wv = tid >> 6;
    const int S = b.samples, NL = b.n_lights, W = b.width, H = b.height;
    const bool owner = wv < G;                          // (wave-uniform) pixel slot q = tid of tile slot wv
    if (tid < 256) thr[tid] = b.gamma_thr[tid];
    if (tid < RTW_LT_MAX * 9) lw[tid] = reinterpret_cast<const uint32_t*>(b.lights)[tid];
    if (tid < 2) qn[tid] = 0u;
    const float4* lnodes = nullptr; int ltop = 0;
    bool staged_done = false;
    int round = 0;                                      // (block-uniform) which of the two queue counters fills; the other one is zero
    Counters ct = { 0, 0, 0, 0, 0, 0 };
    // one walk of the wave: the lanes with `live` cast (O, d, dist); an occluded job sets its bit
    auto walk = [&](bool live, int q, int m, f3 O, f3 d, float dist) {
        Ray ray; ray.o = mk(0, 0, 0); ray.d = mk(0, 0, 1); ray.dist = 0.0f;
        if (live) { ray.o = O; ray.d = d; ray.dist = dist; }
        int hs = -1, hslot = -1, cshape = -1, cslot = -1; f3 pos = mk(0, 0, 0), cpos = mk(0, 0, 0); float seg = ray.dist, cdist = 0.0f;
        lane_find_intersection<false, AN, NT, CAP, (STAGE == 2), true>(sc, cand, lnodes, ltop, STAGE ? staged_shape : -1, ray, live, 0, hs, hslot, pos, seg, cshape, cslot, cpos, cdist, ct);
        if (live && hs >= 0) lds_or(mask, (m >> 5) * NP + q, 1u << (m & 31));
    };
    auto load_pixel = [&](int q, f3& O, f3& n) {
        O = mk(__uint_as_float(lldu(pixw, q)), __uint_as_float(lldu(pixw, NP + q)), __uint_as_float(lldu(pixw, 2 * NP + q)));
        n = mk(__uint_as_float(lldu(pixw, 3 * NP + q)), __uint_as_float(lldu(pixw, 4 * NP + q)), __uint_as_float(lldu(pixw, 5 * NP + q)));
    };
    for (int t0 = (int)blockIdx.x * G; t0 < b.n_tiles; t0 += (int)gridDim.x * G) {          // block-uniform
        // ---- prologue: the owners, a lane per pixel ----
        int fstate = RTW_OC_EMPTY, fpixel = 0; float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f); f3 alb = mk(1.0f, 1.0f, 1.0f);
        if (owner) {
            const int tile = t0 + wv;                   // (a tile slot past the last tile: every pixel outside the frame)
            const int px = (tile % b.tiles_x) * LT_TILE + (lane & 7), py = (tile / b.tiles_x) * LT_TILE + (lane >> 3);
            f3 O = mk(0.0f, 0.0f, 0.0f), n = mk(0.0f, 0.0f, 0.0f);
            if (tile < b.n_tiles && px < W && py < H) {
                fpixel = py * W + px;
                const float4 al = b.albedo[fpixel];
                const int cf = __float_as_int(al.w);
                if (cf != 0) {
                    const float4 gm = b.geom[fpixel];
                    fstate = occlusion_origin(b.cam, px, py, W, H, gm.x, gm.y, gm.z, gm.w, cf, (int)(uint32_t)b.ids[fpixel], b.bias, O, n);
                    acc = b.accum[fpixel];
                    if (b.use_albedo) { const float nf = (float)cf; alb = mk(al.x / nf, al.y / nf, al.z / nf); }
                }
            }
            lstu(pixw, tid, __float_as_uint(O.x)); lstu(pixw, NP + tid, __float_as_uint(O.y)); lstu(pixw, 2 * NP + tid, __float_as_uint(O.z));
            lstu(pixw, 3 * NP + tid, __float_as_uint(n.x)); lstu(pixw, 4 * NP + tid, __float_as_uint(n.y)); lstu(pixw, 5 * NP + tid, __float_as_uint(n.z));
            lstu(pixw, 6 * NP + tid, (uint32_t)fstate); lstu(pixw, 7 * NP + tid, (uint32_t)fpixel);
            lstu(mask, tid, 0u); lstu(mask, NP + tid, 0u);
            const bool any = __ballot(fstate == RTW_OC_CAST) != 0ull;
            if (lane == 0) casts[wv] = any ? 1 : 0;
        }
        __syncthreads();
        bool block_casts = false;
#pragma unroll
        for (int k = 0; k < G; k++) block_casts = block_casts || casts[k] != 0;
        int cnt = __float_as_int(acc.w);
        if (!block_casts) {                             // (whole block) nothing to walk: an OPEN pixel's e per pass, added one by one as the passes would
            if (owner && fstate != RTW_OC_EMPTY) {
                for (int k = 0; k < b.n_passes; k++) { acc.x += alb.x; acc.y += alb.y; acc.z += alb.z; cnt++; }
                const float nf = (float)cnt;
                b.accum[fpixel] = make_float4(acc.x, acc.y, acc.z, __int_as_float(cnt));
                b.argb[fpixel] = pack_pixel(thr, mk(acc.x / nf, acc.y / nf, acc.z / nf));
            }
            __syncthreads();                            // the next tiles' prologue rewrites the pixel words and the flags
            continue;
        }
        if (STAGE && !staged_done) {                    // (whole block) the first tiles with work pay for the tree
            float4* dst = reinterpret_cast<float4*>(gt_dyn + CAP * NT + lt_block_words(NT, COMPACT));
            const float4* src4 = reinterpret_cast<const float4*>(sc->shapes[staged_shape].tnodes);
            for (int i = tid; i < staged_top * 2; i += NT) dst[i] = gld4(src4, (size_t)i);
            lnodes = dst; ltop = staged_top;
            staged_done = true;
            __syncthreads();
        }
        const int n_chunks = NL * S * G;
        for (int k = 0; k < b.n_passes; k++) {
            const int pass = b.first_pass + k;
            for (int base = 0; base < n_chunks; base += LT_ROUND * NW) {                    // block-uniform
                // ---- steps 2 to 5 of every job of the round's chunks; positional: the survivors walk here ----
                for (int c = base + wv; c < n_chunks && c < base + LT_ROUND * NW; c += NW) {    // wave-uniform
                    const int g = c % G, m = c / G, j = m / S, s = m - j * S;
                    if (casts[g] == 0) continue;
                    const int q = g * 64 + lane;
                    f3 O, n, d = mk(0.0f, 0.0f, 1.0f); float dist = 0.0f, t = 0.0f;
                    load_pixel(q, O, n);
                    bool live = false;
                    if (lldu(pixw, 6 * NP + q) == (uint32_t)RTW_OC_CAST) live = lt_job(sc, lw, b.seed, lldu(pixw, 7 * NP + q), pass, j, s, O, n, d, dist, t);
                    if (COMPACT) {
                        const unsigned long long alive = __ballot(live);
                        if (alive != 0ull) {
                            const int leader = __ffsll((long long)alive) - 1;
                            uint32_t at = 0u;
                            if (lane == leader) at = atomicAdd(&qn[round], (uint32_t)__popcll(alive));
                            at = (uint32_t)__shfl((int)at, leader);
                            if (live) lstu(queue, (int)at + __popcll(alive & ((1ull << lane) - 1ull)), (uint32_t)(q << 6 | m));
                        }
                    } else {
                        walk(live, q, m, O, d, dist);
                    }
                }
                if (COMPACT) {
                    // ---- the queue, 64 entries a wave at a time: at most LT_ROUND * NT entries, 64 a chunk ----
                    __syncthreads();
                    const int filled = (int)qn[round];
                    if (tid == 0) qn[round ^ 1] = 0u;   // (nobody fills or reads the other counter before the barrier below)
                    for (int e0 = wv * 64; e0 < filled; e0 += NT) {                         // wave-uniform
                        const bool have = e0 + lane < filled;
                        const uint32_t id = have ? lldu(queue, e0 + lane) : 0u;
                        const int q = (int)(id >> 6), m = (int)(id & 63u), j = m / S, s = m - j * S;
                        f3 O, n, d = mk(0.0f, 0.0f, 1.0f); float dist = 0.0f, t = 0.0f;
                        load_pixel(q, O, n);
                        bool live = false;
                        if (have) live = lt_job(sc, lw, b.seed, lldu(pixw, 7 * NP + q), pass, j, s, O, n, d, dist, t);
                        walk(live, q, m, O, d, dist);
                    }
                    round ^= 1;
                }
                __syncthreads();
            }
            // ---- steps 6 to 8: the owner, in job order ----
            if (owner && fstate != RTW_OC_EMPTY) {
                f3 e = mk(1.0f, 1.0f, 1.0f);
                if (fstate == RTW_OC_CAST) {
                    f3 O, n; load_pixel(tid, O, n);
                    const uint32_t m0 = lldu(mask, tid), m1 = lldu(mask, NP + tid);
                    e = mk(0.0f, 0.0f, 0.0f);
                    for (int j = 0; j < NL; j++) {
                        float sum = 0.0f;
                        for (int s = 0; s < S; s++) {
                            const int m = j * S + s;
                            f3 d; float dist, t;
                            const bool live = lt_job(sc, lw, b.seed, (uint32_t)fpixel, pass, j, s, O, n, d, dist, t);
                            const bool occluded = (((m < 32 ? m0 : m1) >> (m & 31)) & 1u) != 0u;
                            sum += live && !occluded ? t : 0.0f;
                        }
                        const float vis = sum / (float)S;
                        e.x += __uint_as_float(lldu(lw, j * 9 + 5)) * vis; e.y += __uint_as_float(lldu(lw, j * 9 + 6)) * vis; e.z += __uint_as_float(lldu(lw, j * 9 + 7)) * vis;
                    }
                    lstu(mask, tid, 0u); lstu(mask, NP + tid, 0u);
                }
                if (b.use_albedo) { e.x *= alb.x; e.y *= alb.y; e.z *= alb.z; }
                acc.x += e.x; acc.y += e.y; acc.z += e.z; cnt++;
            }
            __syncthreads();                            // the masks are clear before the next pass sets bits
        }
        if (owner && fstate != RTW_OC_EMPTY) {
            const float nf = (float)cnt;
            b.accum[fpixel] = make_float4(acc.x, acc.y, acc.z, __int_as_float(cnt));
            b.argb[fpixel] = pack_pixel(thr, mk(acc.x / nf, acc.y / nf, acc.z / nf));
        }
    }
}
