// rtw_indirect_kernels.h -- one bounce of indirect light from the first-hit feature buffers (rtw_render_indirect; the formula is the header comment
// of include/rtwin.h, its arithmetic rtw_shared.h's occlusion_origin, occlusion_*, indirect_ray and lighting_*).  Included inside rtw_device.hip's
// anonymous namespace after rtw_lighting_kernels.h.  It CALLS lane_find_intersection (ANY false for the gather ray, ANY true for the shadow rays),
// rtw_feature_kernels.h's feature_sample (hit_finish / mesh_finish, the texel carry, material_eval<true>) and the lighting kernel's lt_job, and
// restates none of them.  Independent rays with data-dependent walks: no operand is shared between lanes, so no matrix instruction fits.
//
//   indirect_kernel    ONE launch for all passes of a call.  A block of NT threads owns NT / 4 pixels at a time -- G = NT / 256 tiles of 8 x 8 -- and
//                      takes such tile groups in a grid-stride loop; the prologue, the owners, the staged tree (STAGE, the query kernels' rule) and
//                      the early out for tiles without a casting pixel are lighting_kernel's.  A pass has TWO STAGES with different populations.
//     stage one        the GATHER jobs (pixel, sample s): samples x G chunks of 64, chunk c = sample c / G of the 64 pixels of tile c % G, dealt to
//                      the waves round robin.  The lane makes the ray in registers (indirect_ray), walks it for the CLOSEST hit and finishes that
//                      hit itself: normal, preview colour, texel carry (feature_sample, a Blend drawing from the sample's own stream at counter 1).
//                      It leaves the gather RECORD (O2, m, a_s or the sky colour, c_s) -- 10 words -- in LDS at (field, s, pixel slot), sets bit s of
//                      the pixel's hit word when the ray met a surface, and raises the pass's flag.  A pass whose flag stays down skips stage two.
//     stage two        the LIGHT jobs (pixel, s, light j), job number m = s * n_lights + j < 64: n_lights x samples x G chunks of 64 with s and j
//                      wave-uniform.  A job lives when its gather ray hit and lt_job at (O2, m) passes the cosine test: far fewer than stage one's.
//       COMPACT false  positional: a lane sits where its gather ray sat; the chunk's survivors walk at once, the dead lanes idle.
//       COMPACT true   compacted: the survivors' ids (pixel slot << 6 | m) go to a dense LDS queue -- one ballot, a popcount prefix and ONE atomic add
//                      on an LDS counter per chunk -- in rounds of up to IN_ROUND chunks per wave; after a barrier the waves take 64 entries at a
//                      time and run lt_job again from the record.  Two counters alternate (lighting_kernel's COMPACT).
//     results          an occluded light job sets bit m of its pixel's 64-bit LDS mask (lds_or, an integer: no order of arrival).  After a barrier
//                      the owner folds steps 4 and 5 in job order -- t_j is recomputed from the record, not stored -- adds e to its accumulator
//                      registers and clears its mask and hit word.  ONE read and ONE write of the accumulator entry per call, no float atomic.
//   LDS (words): [CAP * NT candidate lists | 8 x NP pixel words (O, n, state, pixel) | 2 x NP mask words | NP hit words | 10 x samples x NP records |
//   IN_ROUND x NT queue (COMPACT) | staged records], NP = NT / 4, + static: 256 thresholds, 72 light words, G flags, two pass flags, two queue
//   counters.  At 4 samples a 256-thread block holds 16 + 2.75 + 10 KiB (+ 2 KiB queue): five blocks a CU by LDS, where the kernel's registers allow
//   four; at 8 samples 38.75 KiB, still four.  A staging block is IN_STAGED_NT = 512 threads, one a CU -- under __launch_bounds__(1024) the kernel spills
//   VGPRs -- and keeps 128 KiB - 16 - 5.5 - 5 x samples KiB (- 4 KiB queue) for the tree.

#define IN_ROUND 2
#define IN_STAGED_NT 512         // threads of a block that stages a tree: 1024 leave 128 VGPRs a lane, which this kernel does not fit without spilling
__host__ __device__ constexpr int in_block_words(int nt, int samples, bool compact) { return (nt / 4) * (11 + 10 * samples) + (compact ? IN_ROUND * nt : 0); }

struct IndirectBufs {
    const float4* __restrict__ geom;        // (sum normal.xyz, sum depth)
    const float4* __restrict__ albedo;      // (sum rgb, int count)
    const unsigned long long* __restrict__ ids;     // shape in the low word
    float4* __restrict__ accum;             // (sum.xyz, int count)
    uint32_t* __restrict__ argb;
    const float* __restrict__ gamma_thr;
    RtwCamera cam;
    int width, height, tiles_x, n_tiles;
    float bias;
    int samples, n_lights, use_albedo, mirror, carry_on;
    int first_pass, n_passes;
    uint32_t seed;
    RtwLight lights[RTW_LT_MAX];
};

template <bool AN, int NT, int CAP, int STAGE, bool COMPACT>
__global__ __launch_bounds__(NT) void indirect_kernel(const RtwSceneDev* __restrict__ sc, IndirectBufs b, int staged_shape, int staged_top)
{
    static_assert(NT % 256 == 0, "a tile to every four waves");
    constexpr int G = NT / 256, NW = NT / 64, NP = NT / 4;
    HIP_DYNAMIC_SHARED(uint32_t, gt_dyn);               // [CAP * NT candidate words | pixel words | masks | hit words | records | queue | staged records]
    __shared__ float thr[256];
    __shared__ uint32_t lw[RTW_LT_MAX * 9];
    __shared__ int casts[G];
    __shared__ int anyhit[2];
    __shared__ uint32_t qn[2];
    const int S = b.samples, NL = b.n_lights, W = b.width, H = b.height;
    uint32_t* cand = gt_dyn;
    uint32_t* pixw = gt_dyn + CAP * NT; uint32_t* mask = pixw + 8 * NP; uint32_t* hitw = mask + 2 * NP; uint32_t* rec = hitw + NP; uint32_t* queue = rec + 10 * S * NP;
    const int tid = (int)threadIdx.x, lane = lane_id(), wv = tid >> 6;
    const bool owner = wv < G;                          // (wave-uniform) pixel slot q = tid of tile slot wv
    if (tid < 256) thr[tid] = b.gamma_thr[tid];
    if (tid < RTW_LT_MAX * 9) lw[tid] = reinterpret_cast<const uint32_t*>(b.lights)[tid];
    if (tid < 2) { qn[tid] = 0u; anyhit[tid] = 0; }
    const float4* lnodes = nullptr; int ltop = 0;
    bool staged_done = false;
    int round = 0, par = 0;                             // (block-uniform) which queue counter fills and which pass flag is this pass's; the other one is zero
    Counters ct = { 0, 0, 0, 0, 0, 0 };
    // field f of the gather record of sample s of pixel slot q
    auto rec_at = [&](int f, int s, int q) { return (f * S + s) * NP + q; };
    auto load_f3 = [&](const uint32_t* p, int i, int stride) { return mk(__uint_as_float(lldu(p, i)), __uint_as_float(lldu(p, i + stride)), __uint_as_float(lldu(p, i + 2 * stride))); };
    auto store_f3 = [&](uint32_t* p, int i, int stride, f3 v) { lstu(p, i, __float_as_uint(v.x)); lstu(p, i + stride, __float_as_uint(v.y)); lstu(p, i + 2 * stride, __float_as_uint(v.z)); };
    // one any-hit walk of the wave: the lanes with `live` cast (O, d, dist); an occluded job sets its bit
    auto shadow_walk = [&](bool live, int q, int m, f3 O, f3 d, float dist) {
        Ray ray; ray.o = mk(0, 0, 0); ray.d = mk(0, 0, 1); ray.dist = 0.0f;
        if (live) { ray.o = O; ray.d = d; ray.dist = dist; }
        int hs = -1, hslot = -1, cshape = -1, cslot = -1; f3 pos = mk(0, 0, 0), cpos = mk(0, 0, 0); float seg = ray.dist, cdist = 0.0f;
        lane_find_intersection<false, AN, NT, CAP, (STAGE == 2), true>(sc, cand, lnodes, ltop, STAGE ? staged_shape : -1, ray, live, 0, hs, hslot, pos, seg, cshape, cslot, cpos, cdist, ct);
        if (live && hs >= 0) lds_or(mask, (m >> 5) * NP + q, 1u << (m & 31));
    };
    // steps 2 to 5 of lighting at the gather hit of sample s of pixel slot q, for light j (a lane whose gather ray hit)
    auto light_job = [&](int q, int pass, int s, int j, f3& O2, f3& d, float& dist, float& t) {
        O2 = load_f3(rec, rec_at(0, s, q), S * NP);
        const f3 m = load_f3(rec, rec_at(3, s, q), S * NP);
        return lt_job(sc, lw, b.seed, lldu(pixw, 7 * NP + q), pass, j, s, O2, m, d, dist, t);
    };
    for (int t0 = (int)blockIdx.x * G; t0 < b.n_tiles; t0 += (int)gridDim.x * G) {          // block-uniform
        // ---- prologue: the owners, a lane per pixel ----
        int fstate = RTW_OC_EMPTY, fpixel = 0, cnt = 0; f3 acc = mk(0.0f, 0.0f, 0.0f);
        if (owner) {
            const int tile = t0 + wv;                   // (a tile slot past the last tile: every pixel outside the frame)
            const int px = (tile % b.tiles_x) * LT_TILE + (lane & 7), py = (tile / b.tiles_x) * LT_TILE + (lane >> 3);
            f3 O = mk(0.0f, 0.0f, 0.0f), n = mk(0.0f, 0.0f, 0.0f);
            if (tile < b.n_tiles && px < W && py < H) {
                fpixel = py * W + px;
                const int cf = __float_as_int(b.albedo[fpixel].w);
                if (cf != 0) {
                    const float4 gm = b.geom[fpixel];
                    fstate = occlusion_origin(b.cam, px, py, W, H, gm.x, gm.y, gm.z, gm.w, cf, (int)(uint32_t)b.ids[fpixel], b.bias, O, n);
                    const float4 a4 = b.accum[fpixel];
                    acc = mk(a4.x, a4.y, a4.z); cnt = __float_as_int(a4.w);
                }
            }
            store_f3(pixw, tid, NP, O); store_f3(pixw, 3 * NP + tid, NP, n);
            lstu(pixw, 6 * NP + tid, (uint32_t)fstate); lstu(pixw, 7 * NP + tid, (uint32_t)fpixel);
            lstu(mask, tid, 0u); lstu(mask, NP + tid, 0u); lstu(hitw, tid, 0u);
            const bool any = __ballot(fstate == RTW_OC_CAST) != 0ull;
            if (lane == 0) casts[wv] = any ? 1 : 0;
        }
        __syncthreads();
        bool block_casts = false;
#pragma unroll
        for (int k = 0; k < G; k++) block_casts = block_casts || casts[k] != 0;
        if (!block_casts) {                             // (whole block) nothing to walk: an OPEN pixel's zeros, added one by one as the passes would
            if (owner && fstate != RTW_OC_EMPTY) {
                for (int k = 0; k < b.n_passes; k++) { acc.x += 0.0f; acc.y += 0.0f; acc.z += 0.0f; cnt++; }
                const float nf = (float)cnt;
                b.accum[fpixel] = make_float4(acc.x, acc.y, acc.z, __int_as_float(cnt));
                b.argb[fpixel] = pack_pixel(thr, mk(acc.x / nf, acc.y / nf, acc.z / nf));
            }
            __syncthreads();                            // the next tiles' prologue rewrites the pixel words and the flags
            continue;
        }
        if (STAGE && !staged_done) {                    // (whole block) the first tiles with work pay for the tree
            float4* dst = reinterpret_cast<float4*>(gt_dyn + CAP * NT + in_block_words(NT, S, COMPACT));
            const float4* src4 = reinterpret_cast<const float4*>(sc->shapes[staged_shape].tnodes);
            for (int i = tid; i < staged_top * 2; i += NT) dst[i] = gld4(src4, (size_t)i);
            lnodes = dst; ltop = staged_top;
            staged_done = true;
            __syncthreads();
        }
        const int n_gather = S * G, n_chunks = NL * S * G;
        for (int k = 0; k < b.n_passes; k++) {
            const int pass = b.first_pass + k;
            // ---- stage one: the gather rays, closest hit; the lane finishes its hit and leaves the record ----
            for (int c = wv; c < n_gather; c += NW) {   // wave-uniform
                const int g = c % G, s = c / G;
                if (casts[g] == 0) continue;
                const int q = g * 64 + lane;
                const bool casting = lldu(pixw, 6 * NP + q) == (uint32_t)RTW_OC_CAST;
                const uint32_t pixel = lldu(pixw, 7 * NP + q);
                const f3 O = load_f3(pixw, q, NP), n = load_f3(pixw, 3 * NP + q, NP);
                f3 d = mk(0.0f, 0.0f, 1.0f); float cs = 0.0f;
                bool have = false;
                if (casting) {
                    f3 v = mk(0.0f, 0.0f, 0.0f), w = mk(0.0f, 0.0f, 0.0f);
                    if (b.mirror) {
                        const int py = (int)pixel / W;
                        w = pinhole_direction(b.cam, (int)pixel - py * W, py, W, H);
                    } else {
                        const size_t i = (size_t)occlusion_table_index(b.seed, pixel, (uint32_t)pass, (uint32_t)s) * 3;
                        const float* e = sc->unit_table;
                        v = mk(gld1(e, i), gld1(e, i + 1), gld1(e, i + 2));
                    }
                    have = indirect_ray(v, w, n, b.mirror != 0, d, cs);
                }
                if (casting) lstu(rec, rec_at(9, s, q), __float_as_uint(cs));
                Ray ray; ray.o = mk(0, 0, 0); ray.d = mk(0, 0, 1); ray.dist = 0.0f;
                if (have) { ray.o = O; ray.d = d; ray.dist = 1000.0f; }
                FeatureHit fh;
                fh.shape = -1; fh.slot = -1; fh.carry_shape = -1; fh.carry_slot = -1; fh.pos = mk(0, 0, 0); fh.carry_pos = mk(0, 0, 0); fh.seg = ray.dist; fh.carry_dist = 0.0f;
                lane_find_intersection<false, AN, NT, CAP, (STAGE == 2), false>(sc, cand, lnodes, ltop, STAGE ? staged_shape : -1, ray, have, 0, fh.shape, fh.slot, fh.pos, fh.seg,
                                                                                 fh.carry_shape, fh.carry_slot, fh.carry_pos, fh.carry_dist, ct);
                if (casting) {
                    f3 m = mk(0.0f, 0.0f, 0.0f), a = mk(0.0f, 0.0f, 0.0f), O2 = mk(0.0f, 0.0f, 0.0f);      // no ray (mirror, grazing): L_s = 0, c_s = 0
                    if (have) {
                        PathRng rng;
                        rng.key = stream_key(b.seed, pixel, ((uint32_t)pass * 64u + (uint32_t)s) | RTW_OCCLUSION_STREAM); rng.counter = 1u;
                        rng.table_base = 0; rng.table_reads = 0; rng.pre_reads = 0xFFFFFFFFu; rng.pre_x = rng.pre_y = rng.pre_z = 0.0f;
                        float depth; int shape, tri;
                        feature_sample<AN>(sc, b.carry_on, ray, rng, fh, m, depth, a, shape, tri);
                        if (fh.shape >= 0) {
                            O2 = mk(fh.pos.x + m.x * b.bias, fh.pos.y + m.y * b.bias, fh.pos.z + m.z * b.bias);
                            lds_or(hitw, q, 1u << s);
                            anyhit[par] = 1;
                        }
                    }
                    store_f3(rec, rec_at(0, s, q), S * NP, O2); store_f3(rec, rec_at(3, s, q), S * NP, m); store_f3(rec, rec_at(6, s, q), S * NP, a);
                }
            }
            __syncthreads();
            const bool lit = NL > 0 && anyhit[par] != 0;   // (block-uniform) a pass whose gather rays all missed casts no shadow ray
            if (tid == 0) anyhit[par ^ 1] = 0;          // (nobody raises or reads the other flag before the next pass's stage one)
            par ^= 1;
            // ---- stage two: the light jobs at the gather hits, any hit ----
            for (int base = 0; lit && base < n_chunks; base += IN_ROUND * NW) {                  // block-uniform
                for (int c = base + wv; c < n_chunks && c < base + IN_ROUND * NW; c += NW) {    // wave-uniform
                    const int g = c % G, m = c / G, s = m / NL, j = m - s * NL;
                    if (casts[g] == 0) continue;
                    const int q = g * 64 + lane;
                    f3 O2 = mk(0.0f, 0.0f, 0.0f), d = mk(0.0f, 0.0f, 1.0f); float dist = 0.0f, t = 0.0f;
                    bool live = false;
                    if ((lldu(hitw, q) >> s) & 1u) live = light_job(q, pass, s, j, O2, d, dist, t);
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
                        shadow_walk(live, q, m, O2, d, dist);
                    }
                }
                if (COMPACT) {
                    // ---- the queue, 64 entries a wave at a time: at most IN_ROUND * NT entries, 64 a chunk ----
                    __syncthreads();
                    const int filled = (int)qn[round];
                    if (tid == 0) qn[round ^ 1] = 0u;   // (nobody fills or reads the other counter before the barrier below)
                    for (int e0 = wv * 64; e0 < filled; e0 += NT) {                         // wave-uniform
                        const bool have = e0 + lane < filled;
                        const uint32_t id = have ? lldu(queue, e0 + lane) : 0u;
                        const int q = (int)(id >> 6), m = (int)(id & 63u), s = m / NL, j = m - s * NL;
                        f3 O2 = mk(0.0f, 0.0f, 0.0f), d = mk(0.0f, 0.0f, 1.0f); float dist = 0.0f, t = 0.0f;
                        bool live = false;
                        if (have) live = light_job(q, pass, s, j, O2, d, dist, t);
                        shadow_walk(live, q, m, O2, d, dist);
                    }
                    round ^= 1;
                }
                __syncthreads();
            }
            // ---- steps 4 to 6: the owner, in job order ----
            if (owner && fstate != RTW_OC_EMPTY) {
                f3 e = mk(0.0f, 0.0f, 0.0f);
                if (fstate == RTW_OC_CAST) {
                    const uint32_t m0 = lldu(mask, tid), m1 = lldu(mask, NP + tid), hits = lldu(hitw, tid);
                    f3 A = mk(0.0f, 0.0f, 0.0f); float Wt = 0.0f;
                    for (int s = 0; s < S; s++) {
                        f3 L = load_f3(rec, rec_at(6, s, tid), S * NP);           // a_s, or the sky colour of a miss
                        const float cs = __uint_as_float(lldu(rec, rec_at(9, s, tid)));
                        if ((hits >> s) & 1u) {
                            f3 E = mk(0.0f, 0.0f, 0.0f);
                            for (int j = 0; j < NL; j++) {
                                const int m = s * NL + j;
                                f3 O2, d; float dist, t;
                                const bool live = light_job(tid, pass, s, j, O2, d, dist, t);
                                const bool occluded = (((m < 32 ? m0 : m1) >> (m & 31)) & 1u) != 0u;
                                const float tj = live && !occluded ? t : 0.0f;
                                E.x += __uint_as_float(lldu(lw, j * 9 + 5)) * tj; E.y += __uint_as_float(lldu(lw, j * 9 + 6)) * tj; E.z += __uint_as_float(lldu(lw, j * 9 + 7)) * tj;
                            }
                            L = mk(L.x * E.x, L.y * E.y, L.z * E.z);
                        }
                        A.x += L.x * cs; A.y += L.y * cs; A.z += L.z * cs; Wt += cs;
                    }
                    if (Wt > 0.0f) e = mk(A.x / Wt, A.y / Wt, A.z / Wt);
                    if (b.use_albedo) {                 // (the feature entry again rather than three registers held through every walk)
                        const float4 al = b.albedo[fpixel];
                        const float nf = (float)__float_as_int(al.w);
                        e.x *= al.x / nf; e.y *= al.y / nf; e.z *= al.z / nf;
                    }
                    lstu(mask, tid, 0u); lstu(mask, NP + tid, 0u); lstu(hitw, tid, 0u);
                }
                acc.x += e.x; acc.y += e.y; acc.z += e.z; cnt++;
            }
            __syncthreads();                            // the records, masks and hit words are free before the next pass writes them
        }
        if (owner && fstate != RTW_OC_EMPTY) {
            const float nf = (float)cnt;
            b.accum[fpixel] = make_float4(acc.x, acc.y, acc.z, __int_as_float(cnt));
            b.argb[fpixel] = pack_pixel(thr, mk(acc.x / nf, acc.y / nf, acc.z / nf));
        }
    }
}
