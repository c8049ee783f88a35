// rtw_feature_kernels.h -- first-hit feature buffers (rtw_render_features): per pixel the depth, shading normal, base colour and ids of what its
// camera rays meet first, accumulated over sub-samples and passes the way the image is.  Included inside rtw_device.hip's anonymous namespace after
// rtw_group_kernels.h; it CALLS that file's and rtw_wave_kernels.h's device functions (camera_ray_xy, bins_walk_rays, packet_walk, analytic_test,
// hit_finish / mesh_finish, material_eval<true>) and restates none of them.
//
// A sample (pixel, pass k, sub-sample i) is the camera ray the render kernels build for it; FindIntersectionWithScene of that ray gives
//   depth  = Result.Distance (a miss: the ray's own 1000)        normal = Result.HitNormal (a miss: 0, 0, 0)
//   albedo = RayTrace(ray, 1, RenderOption{UseBaseColor}) = PreviewColor(Result) * Result.SampledColor (a miss: the sky colour)
//   shape, triangle = what rtw_trace_closest reports (a miss: -1, -1)
// Per pass each of the seven float channels takes c = (v_0 + ... + v_{ns-1}) / ns (left to right from +0, no division when ns == 1), then
// sum += c, count += 1 in pass order (AccumulatePixel::AddPixel).  The ids are those of sub-sample 0 of the call's last pass.
//
//   gfeature_sky_kernel  sky-only tiles: a lane per pixel, all passes and sub-samples of the call in a row, the sums in registers (gsky_kernel's shape)
//   gfeature_kernel      a wave per busy tile, a lane per pixel: the call's (pass, sub-sample) pairs in order, up to four at a time -- through
//                        bins_walk_rays where the scene is one mesh with bins and all the wave's rays are tame, through the per-shape loop of
//                        gprimary_kernel otherwise.  No path state, no workspace, no lists: the sums stay in registers and are stored once.
//
// The per-shape loop (feature_find) is a COPY of the one inside gprimary_kernel (rtw_group_kernels.h) without its counters, not a helper lifted out of
// it: that loop is written into the kernel's body, and no existing kernel's code object may move for this one.

struct FeatureBufs {
    float4* __restrict__ geom;      // [pixels] sum of normal.xyz, sum of depth
    float4* __restrict__ albedo;    // [pixels] sum of albedo.rgb, int count in the bits of w (the accumulator's layout)
    unsigned long long* __restrict__ ids;   // [pixels] shape in the low word, triangle in the high word: int32 x 2 in memory
};

// the running sums of one pixel: the call's (`s*`, cnt) and the pass at hand (`c*`)
struct FeatureAcc {
    f3 sn, sa; float sd; int cnt;
    f3 cn, ca; float cd;
    int shape, tri;
};
__device__ __forceinline__ void feature_load(FeatureAcc& a, const FeatureBufs& fb, int pixel)
{
    const float4 ga = fb.geom[pixel], aa = fb.albedo[pixel];
    a.sn = mk(ga.x, ga.y, ga.z); a.sd = ga.w; a.sa = mk(aa.x, aa.y, aa.z); a.cnt = __float_as_int(aa.w);
    a.cn = mk(0, 0, 0); a.ca = mk(0, 0, 0); a.cd = 0.0f;
    a.shape = -1; a.tri = -1;
}
// sub-sample i of ns: v joins the pass value; after the last one the pass value joins the sums (AddPixel)
__device__ __forceinline__ void feature_add(FeatureAcc& a, f3 n, float depth, f3 alb, int i, int ns)
{
    a.cn = a.cn + n; a.cd = a.cd + depth; a.ca = a.ca + alb;
    if (i != ns - 1) return;
    if (ns != 1) { a.cn = a.cn / (float)ns; a.cd = a.cd / (float)ns; a.ca = a.ca / (float)ns; }
    a.sn = a.sn + a.cn; a.sd = a.sd + a.cd; a.sa = a.sa + a.ca; a.cnt++;
    a.cn = mk(0, 0, 0); a.ca = mk(0, 0, 0); a.cd = 0.0f;
}
__device__ __forceinline__ void feature_store(const FeatureAcc& a, const FeatureBufs& fb, int pixel)
{
    fb.geom[pixel] = make_float4(a.sn.x, a.sn.y, a.sn.z, a.sd);
    fb.albedo[pixel] = make_float4(a.sa.x, a.sa.y, a.sa.z, __int_as_float(a.cnt));
    fb.ids[pixel] = (unsigned long long)(uint32_t)a.shape | ((unsigned long long)(uint32_t)a.tri << 32);
}

// ---- sky-only tiles ---------------------------------------------------------------------------------------------------------------
template <bool CAM>
__global__ __launch_bounds__(256) void gfeature_sky_kernel(FeatureBufs fb, RtwGroupParams g)
{
    const RtwRenderParams& p = g.rp;
    const int npix = p.width * p.height;
    const uint32_t phase = table_phase(p.seed);
    const int wave0 = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), nwaves = (int)(gridDim.x * (blockDim.x >> 6));
    for (int wk = wave0; wk < g.n_sky; wk += nwaves) {
        const int wt = (int)cldu(g.sky_tiles, wk);
        int px = 0, py = 0;
        if (!group_xy(g, wt, lane_id(), px, py)) continue;
        const int pixel = py * p.width + px;
        FeatureAcc a; feature_load(a, fb, pixel);
        for (int k = 0; k < g.n_passes; k++) {
            for (int i = 0; i < p.sub_samples; i++) {
                PathRng rng; rng_init(rng, p.seed, phase, (uint64_t)npix, (uint32_t)pixel, (uint32_t)(g.first_pass + k), (uint32_t)i);
                const Ray ray = camera_ray_xy<CAM>(p, px, py, i, rng);          // (d.y for the sky colour and dist, the constant 1000, for the depth: the rest of the ray is dead code)
                feature_add(a, mk(0, 0, 0), ray.dist, sky_color(ray.d.y), i, p.sub_samples);
            }
        }
        feature_store(a, fb, pixel);
    }
}

// ---- busy tiles -------------------------------------------------------------------------------------------------------------------
// What FindIntersectionWithScene leaves behind for one ray, as gprimary_kernel records it: the hit (shape < 0: none), and for scenes with analytic
// shapes the mesh hit whose sampled colour a later sphere / plane / capsule-side / RTriangle hit of the same query keeps.
struct FeatureHit { int shape, slot, carry_shape, carry_slot; f3 pos, carry_pos; float seg, carry_dist; };

// FindIntersectionWithScene of the wave's camera rays (Src/RayTracerScene.cpp:99-125), shapes in insertion order, a ray per lane: the per-shape loop of
// gprimary_kernel (analytic_test / packet_walk / the per-lane walk of the tile's bin; the tests as written for the rays that are not tame).  The whole
// wave calls it together; a lane without a pixel (`live` false) takes part in the cross-lane operations and tests nothing.
template <bool AN>
__device__ __forceinline__ void feature_find(const RtwSceneDev* __restrict__ sc, const RtwRenderParams& p, const Ray& ray, bool live, int lane, int bin, bool prune, FeatureHit& fh)
{
    Counters ct = { 0, 0, 0, 0, 0, 0 };
    const int n_shapes = sc->n_shapes;
    fh.shape = -1; fh.slot = -1; fh.carry_shape = -1; fh.carry_slot = -1;
    fh.pos = mk(0, 0, 0); fh.carry_pos = mk(0, 0, 0);
    fh.seg = ray.dist; fh.carry_dist = 0.0f;
    const bool tame = ray_is_tame(ray);
    const bool any_untame = __ballot(live && !tame) != 0ull;
    const bool skx = near_zero(ray.d.x), sky = near_zero(ray.d.y), skz = near_zero(ray.d.z);
    for (int k = 0; k < n_shapes; k++) {
        const RtwShapeDev& sh = sc->shapes[k];
        const int kind = AN ? sh.kind : RTW_SHAPE_MESH;
        float t0, t1;
        const bool inbox = live && ((AN && kind == RTW_SHAPE_PLANE) ||      // a plane has no culling box (RPlane::HasCullingBounds)
                                    slab_exact(ray, sh.bmin[0], sh.bmin[1], sh.bmin[2], sh.bmax[0], sh.bmax[1], sh.bmax[2], t0, t1));
        if (__ballot(inbox) == 0ull) continue;
        float cur = fh.seg; f3 pos = mk(0, 0, 0); int slot_hit = -1;
        bool any = false;
        const uint32_t* __restrict__ boff = p.bins[k].off;
        if (AN && kind != RTW_SHAPE_MESH) {          // a sphere / plane / capsule / triangle: every lane tests its own ray; slot = the part hit
            if (inbox) any = analytic_test(sh, ray, fh.seg, pos, cur, slot_hit);
        } else if (boff == nullptr) {                // no bins for this shape: packet walk of its tree
            any = packet_walk<false, false>(sh.nodes, sh.tris, sh.n_nodes, ray, inbox && tame, prune, cur, pos, slot_hit, ct);
            if (any_untame) {
                const bool a2 = packet_walk<false, true>(sh.nodes, sh.tris, sh.n_nodes, ray, inbox && !tame, false, cur, pos, slot_hit, ct);
                any = any || a2;
            }
        } else {
            const bool active = inbox && tame;
            const bool active_exact = inbox && !tame;
            const uint32_t* __restrict__ bent = p.bins[k].ent;
            const int e0 = (int)cldu(boff, bin), e1 = (int)cldu(boff, bin + 1);
            const float4* nd4 = reinterpret_cast<const float4*>(sh.nodes);
            const float4* tr4 = reinterpret_cast<const float4*>(sh.tris);
            const float ix = (!tame && skx) ? 0.0f : 1.0f / ray.d.x, iy = (!tame && sky) ? 0.0f : 1.0f / ray.d.y, iz = (!tame && skz) ? 0.0f : 1.0f / ray.d.z;
            const float eps_t = 2.0e-5f * fmaxf(fabsf(ix), fmaxf(fabsf(iy), fabsf(iz)));
            bool clip = prune && seg_clips(cur);         // (an earlier shape's hit may have left a segment the clip does not hold for)
            for (int ec = e0; ec < e1; ec += 64) {
                const int cnt = e1 - ec < 64 ? e1 - ec : 64;
                const int mnode = lane < cnt ? (int)bent[ec + lane] : 0;
                const float4 mlo = gld4(nd4, 2 * (size_t)mnode), mhi = gld4(nd4, 2 * (size_t)mnode + 1);
                const int mleaf = __float_as_int(mhi.w) < 0 ? 0 : __float_as_int(mhi.w);
                const float4 ta = gld4(tr4, 4 * (size_t)mleaf), tb = gld4(tr4, 4 * (size_t)mleaf + 1), tc = gld4(tr4, 4 * (size_t)mleaf + 2);
                const float td = gld4(tr4, 4 * (size_t)mleaf + 3).x;
                for (int j = 0; j < cnt; j++) {
                    const float lox = readlane_f(mlo.x, j), loy = readlane_f(mlo.y, j), loz = readlane_f(mlo.z, j);
                    const float hix = readlane_f(mhi.x, j), hiy = readlane_f(mhi.y, j), hiz = readlane_f(mhi.z, j);
                    const float x1 = (lox - ray.o.x) * ix, x2 = (hix - ray.o.x) * ix;
                    const float y1 = (loy - ray.o.y) * iy, y2 = (hiy - ray.o.y) * iy;
                    const float z1 = (loz - ray.o.z) * iz, z2 = (hiz - ray.o.z) * iz;
                    const float tmin = fmaxf(fmaxf(fminf(x1, x2), fminf(y1, y2)), fminf(z1, z2));
                    const float tmax = fminf(fminf(fmaxf(x1, x2), fmaxf(y1, y2)), fmaxf(z1, z2));
                    bool hit = active && (tmax > tmin);
                    if (clip) hit = hit && !(tmin > cur + (eps_t + 1.0e-4f * cur)) && !(tmax < -eps_t);
                    if (any_untame) {                // wave-uniform: RRay::TestIntersectionWithAabb as written for the lanes that need it
                        float emin = -FLT_MAX, emax = FLT_MAX;
                        if (!skx) { emin = ref_max(emin, ref_min(x1, x2)); emax = ref_min(emax, ref_max(x1, x2)); }
                        if (!sky) { emin = ref_max(emin, ref_min(y1, y2)); emax = ref_min(emax, ref_max(y1, y2)); }
                        if (!skz) { emin = ref_max(emin, ref_min(z1, z2)); emax = ref_min(emax, ref_max(z1, z2)); }
                        if (active_exact) hit = emax > emin;
                    }
                    if (__ballot(hit) == 0ull) continue;
                    const int leaf = __builtin_amdgcn_readlane(mleaf, j);
                    const float4 a = make_float4(readlane_f(ta.x, j), readlane_f(ta.y, j), readlane_f(ta.z, j), readlane_f(ta.w, j));
                    const float4 bq = make_float4(readlane_f(tb.x, j), readlane_f(tb.y, j), readlane_f(tb.z, j), readlane_f(tb.w, j));
                    const float4 c = make_float4(readlane_f(tc.x, j), readlane_f(tc.y, j), readlane_f(tc.z, j), readlane_f(tc.w, j));
                    const float d1 = readlane_f(td, j);
                    if (hit) {
                        f3 cp; float dist;
                        if (triangle_test(ray, cur, a, bq, c, d1, cp, dist)) { cur = dist; pos = cp; slot_hit = leaf; any = true; clip = clip && seg_clips(dist); }
                    }
                }
            }
        }
        if (any) {
            fh.seg = cur; fh.shape = k; fh.slot = slot_hit; fh.pos = pos;
            if (AN && kind == RTW_SHAPE_MESH) { fh.carry_shape = k; fh.carry_slot = slot_hit; fh.carry_pos = pos; fh.carry_dist = cur; }
            else if (AN && slot_hit != 0) fh.carry_shape = -1;      // a capsule end resets the sampled colour (Src/Shapes.cpp:34-62)
        }
    }
}

// one sample's values from its recorded hit (a live lane's): the RayHitResult (hit_finish / mesh_finish, the shared-result colour inheritance as
// group_shade_step applies it) and the preview evaluation of the material tree, which may draw from the path's stream (Blend)
template <bool AN>
__device__ __forceinline__ void feature_sample(const RtwSceneDev* __restrict__ sc, int carry_on, const Ray& ray, PathRng& rng, const FeatureHit& fh,
                                               f3& normal, float& depth, f3& alb, int& shape, int& tri)
{
    shape = fh.shape; tri = -1;
    if (fh.shape < 0) { normal = mk(0, 0, 0); depth = ray.dist; alb = sky_color(ray.d.y); return; }
    const TravCtx tc = make_trav();
    Counters none = { 0, 0, 0, 0, 0, 0 };
    const RtwShapeDev& sh = sc->shapes[fh.shape];
    Hit h;
    if (AN) {
        hit_finish<false>(sc, sh, tc, fh.pos, fh.seg, fh.slot, h, tri, none);
        if (carry_on && sh.kind != RTW_SHAPE_MESH && fh.slot == 0 && fh.carry_shape >= 0) {
            Hit hc; int ti;
            mesh_finish<false>(sc, sc->shapes[fh.carry_shape], tc, fh.carry_pos, fh.carry_dist, fh.carry_slot, hc, ti, none);
            h.color = hc.color; h.alpha = hc.alpha;
        }
    } else {
        mesh_finish<false>(sc, sh, tc, fh.pos, fh.seg, fh.slot, h, tri, none);
    }
    normal = h.normal; depth = h.dist;
    if (!sh.has_material) { alb = mk(0, 0, 0); return; }
    Ray out = ray;
    const Bounce pv = material_eval<true>(sc, sh, ray, h, out, rng);
    alb = mk(0, 0, 0) + pv.att * h.color;
}

template <bool AN, bool CAM, bool LENS>
__global__ __launch_bounds__(256) void gfeature_kernel(const RtwSceneDev* __restrict__ sc, FeatureBufs fb, RtwGroupParams g, int carry_on)
{
    const RtwRenderParams& p = g.rp;
    const int npix = p.width * p.height;
    const uint32_t phase = table_phase(p.seed);
    const bool prune = sc->prune != 0;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    if (wave >= (uint32_t)g.n_busy) return;              // (whole waves: nothing below is a block-level operation)
    const int wt = g.busy_tiles ? (int)cldu(g.busy_tiles, (int)wave) : g.first_tile + (int)wave;
    const int lane = lane_id();
    int px = 0, py = 0;
    const bool live = group_xy(g, wt, lane, px, py);
    if (!live) { px = 0; py = 0; }
    const int pixel = live ? py * p.width + px : 0;
    // the wave's bin, as gprimary_kernel finds it: all its pixels lie in one tile of the screen's bin grid
    int bin = 0;
    if (__ballot(live) != 0ull) {
        int tx = 0, ty = 0;
        (void)work_to_xy(p, wt * 64, tx, ty);
        bin = (ty >> (6 - p.tile_shift)) * p.tiles_per_row + (tx >> p.tile_shift);
    }
    FeatureAcc acc;
    if (live) feature_load(acc, fb, pixel);
    else { acc.sn = acc.sa = acc.cn = acc.ca = mk(0, 0, 0); acc.sd = acc.cd = 0.0f; acc.cnt = 0; acc.shape = acc.tri = -1; }
    const int ns = p.sub_samples, total = g.n_passes * ns, last_k = g.n_passes - 1;
    // one mesh with bins: the bin is walked once for up to four of the call's ray sets
    const bool one_mesh = !LENS && !AN && sc->n_shapes == 1 && p.bins[0].off != nullptr;
    for (int q0 = 0; q0 < total; q0 += 4) {                  // ray sets q = k * ns + i in order, four at a time
        const int nr = total - q0 < 4 ? total - q0 : 4;
        float w_cur[4] = { 0.f, 0.f, 0.f, 0.f }; f3 w_pos[4]; int w_slot[4] = { -1, -1, -1, -1 }; bool w_any[4] = { false, false, false, false };
#pragma unroll
        for (int r = 0; r < 4; r++) w_pos[r] = mk(0, 0, 0);
        bool shared_walk = false;
        if (one_mesh) {
            f3 w_d[4]; bool w_act[4]; bool all_tame = true;
            const RtwShapeDev& sh = sc->shapes[0];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                w_d[r] = mk(0, 0, -1); w_act[r] = false;
                if (r < nr) {
                    const int k = (q0 + r) / ns, i = (q0 + r) - k * ns;
                    PathRng rng; rng_init(rng, p.seed, phase, (uint64_t)npix, (uint32_t)pixel, (uint32_t)(g.first_pass + k), (uint32_t)i);
                    const Ray ray = camera_ray_xy<CAM>(p, px, py, i, rng);
                    float t0, t1;
                    w_d[r] = ray.d; w_cur[r] = ray.dist;
                    w_act[r] = live && slab_exact(ray, sh.bmin[0], sh.bmin[1], sh.bmin[2], sh.bmax[0], sh.bmax[1], sh.bmax[2], t0, t1);
                    all_tame = all_tame && (!live || ray_is_tame(ray));
                }
            }
            if (__ballot(!all_tame) == 0ull) {
                Counters none = { 0, 0, 0, 0, 0, 0 };
                shared_walk = true;
                bins_walk_rays<false>(sh, p.bins[0].off, p.bins[0].ent, bin, lane, nr, prune, camera_eye<CAM>(p.cam), w_d, w_act, w_cur, w_pos, w_slot, w_any, none);
            }
        }
        for (int r = 0; r < nr; r++) {                       // wave-uniform loop
            const int k = (q0 + r) / ns, i = (q0 + r) - k * ns;
            const int pass = g.first_pass + k;
            PathRng rng; rng_init(rng, p.seed, phase, (uint64_t)npix, (uint32_t)pixel, (uint32_t)pass, (uint32_t)i);
            const Ray ray = camera_ray_xy<CAM, LENS>(p, px, py, i, rng, (uint32_t)pass);
            FeatureHit fh;
            if (shared_walk) {                               // the walk above found this ray's closest hit
                const bool any = r == 0 ? w_any[0] : (r == 1 ? w_any[1] : (r == 2 ? w_any[2] : w_any[3]));
                fh.shape = any ? 0 : -1;
                fh.slot = r == 0 ? w_slot[0] : (r == 1 ? w_slot[1] : (r == 2 ? w_slot[2] : w_slot[3]));
                fh.pos = mk(pick4(r, w_pos[0].x, w_pos[1].x, w_pos[2].x, w_pos[3].x), pick4(r, w_pos[0].y, w_pos[1].y, w_pos[2].y, w_pos[3].y),
                            pick4(r, w_pos[0].z, w_pos[1].z, w_pos[2].z, w_pos[3].z));
                fh.seg = pick4(r, w_cur[0], w_cur[1], w_cur[2], w_cur[3]);
                fh.carry_shape = -1; fh.carry_slot = -1; fh.carry_pos = mk(0, 0, 0); fh.carry_dist = 0.0f;
            } else {
                feature_find<AN>(sc, p, ray, live, lane, bin, prune, fh);
            }
            if (live) {
                f3 n, alb; float depth; int shape, tri;
                feature_sample<AN>(sc, carry_on, ray, rng, fh, n, depth, alb, shape, tri);
                if (i == 0 && k == last_k) { acc.shape = shape; acc.tri = tri; }
                feature_add(acc, n, depth, alb, i, ns);
            }
        }
    }
    if (live) feature_store(acc, fb, pixel);
}
