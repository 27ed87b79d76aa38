// pca_k1.hip -- K1  kitti_project_sample_filter for gfx950 (MI355X)
//   fused  velo2frame -> velo2img (frustum mask) -> nearest sample of semseg + RGB -> class filter -> stable append
//   (sem_pc_accum.py:317-402, kitti360_sem_pc_accum.py:132-156 of the reference), one launch for a batch of frames.
//
// What bounds it (measured): per frame the kernel moves 1.9 MB of points, the image lines its ~60 k gathers
// touch and 1 MB of kept records; it does ~30 f64 operations for the 29 % of the points that fall into the frustum.
// On scattered points the batch form is bound by its GATHERS, not by HBM: a wave-wide gather pulls 64 distinct lines
// through the CU's L1 for 64 x (1 or 4) useful bytes (with every gather at pixel 0 the front kernel runs in 31 us instead
// of 57; without phase 2 at all in 23 us = 5.3 TB/s).  So the design is about (1) not fetching an image into eight L2s,
// (2) not spending vector issue slots on the 71 % of the points that are outside the frustum, (3) as few gathered lines
// as the reference's semantics allow, (4) enough independent workgroups in flight to cover the chain
// descriptor -> points -> class gather -> colour gather -> stores, with every link a single round trip.
//
//   * one workgroup = one tile of BLK*PPT consecutive points of one frame.
//   * phase 1 (every point): 16-byte load, f32 estimate of the three projection rows with a certified error bound,
//     conservative frustum test -> candidates (a superset of the in-frustum points), compacted into an LDS list.
//   * phase 2 (candidates only, dense lanes): the exact f64 path -- fma chain, IEEE divide, rint, 6-way mask -- two
//     gathers (class byte, one unaligned dword for r,g,b), 256-bit class filter from LDS.  The rounds of a tile are
//     software-pipelined: all point re-loads, then all projections and gathers, then all filters; no sweep consumes what
//     it gathers, so the gathers of all rounds of a wave are in flight together.  Batches gather the colour after the
//     class filter, for the kept points only (24 % fewer colour gathers; one frame gathers both at once: latency).
//   * stable compaction inside the tile: ballot ranks + one 64-lane DPP scan per workgroup.
//   * across tiles, two forms:
//       FUSED (a launch of at most one tile per CU: every workgroup is resident, tile = blockIdx): decoupled
//         look-back (8-byte {flag, epoch, value} granules, relaxed agent-scope atomics, bounded spin), then the SoA
//         stores of the kept records.  One launch: this is what integrate() of one frame runs.
//       SPLIT (batches): no workgroup ever waits for another.  The front kernel writes each tile's kept records
//         (x, y, z, intensity as loaded + rgb | class: 20 B per kept point) and its count; k1_append adds up the counts
//         before its tile and streams the records into the SoA store, fully coalesced.  Grid x = queue, queue q holding
//         the frames f = q (mod Q): with the round-robin placement of workgroups on the 8 XCDs a frame's image lines are
//         pulled into ONE L2 instead of eight (placement is a speed matter only, nothing depends on it).  The frame
//         descriptor comes through the scalar cache from a closed-form index (no dependent vector loads).
//     Measured on 64 x 120 k points: chaining the tiles inside one launch -- tickets + look-back over all
//     tiles (round 1), or per-frame sums of published counts + frame totals (round 3, 'LINKED') -- makes every tile wait
//     for the slowest of the ~1000 tiles in flight before it may store (10 us of a 24 us tile lifetime): 107 us against
//     72 for the split form, which pays 20 B written + 20 B read per kept point instead and never waits.
// Host side: one K1Call (what a call's plans share) and one K1Plan per launch -- FUSED one; SPLIT (512 x 4 tiles) one per sub-batch
// (k1_cut_batches), all over ONE workspace (k1_ws_layout).  Kernels by table; every PCA_K1_* switch is read in k1_tuning.
#include "pca_common.h"
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pca_k1_body.h"

template <int BLK, int PPT, bool SPLIT, bool BILIN>
__global__ __launch_bounds__(BLK) void k1_kitti(const K1Args a) { k1_body<BLK, PPT, SPLIT, BILIN, false>(a); }

// same, with the frame descriptors in the kernel arguments (no upload before the launch): equal-sized frames, <= 64 of them
template <int BLK, int PPT, bool BILIN>
__global__ __launch_bounds__(BLK) void k1_kitti_inl(const K1Args a, const K1InlineFrames inl) { k1_body<BLK, PPT, true, BILIN, true>(a); }


// SPLIT, second kernel: streams a tile's kept records into the SoA store (consecutive lanes write consecutive
// records: every store instruction is fully coalesced).  The tile's store offset is the sum of the counts of the
// tiles before it, which every workgroup adds up for itself (<= K1_MAX_SPLIT_TILES values from L2: no scan kernel,
// no atomics, nobody waits); the last tile of a frame also closes the frame's segment.
#define K1_MAX_SPLIT_TILES 16384
struct K1AppendArgs {
    const float4 *rec_p;
    const uint32_t *rec_c;
    const uint32_t *counts;
    const int32_t *lastf;
    int tile_points;
    int tiles;                 // tiles of the (sub-)batch
    int group;                 // consecutive tiles per workgroup
    pca_store st;
    int64_t *frame_off;
    int first_slot;
    uint32_t *status;
};

// A workgroup takes `group` consecutive tiles (round 5; one before): the sum over the counts in front of it is taken once per
// group -- tile 15 000 of a 64-frame batch reads 60 KB of counts before its first store, and 15 000 workgroups did that --
// and the staging records, written once by the front kernel and read once here, are read with the non-temporal hint, the SoA
// stores (nobody re-reads them before the raster's next pass over the whole store) likewise when `nt` says so.
template <bool NT>
__device__ __forceinline__ void k1_append_body(const K1AppendArgs &a)
{
    constexpr int BLK = K1_APPEND_BLK;
    const int tile0 = (int)blockIdx.x * a.group;
    const int tile1 = tile0 + a.group < a.tiles ? tile0 + a.group : a.tiles;
    __shared__ uint32_t s_w[BLK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t sum = 0;
    for (int t = threadIdx.x; t < tile0; t += BLK) sum += pca_ldg(a.counts + t);
    sum = wave_reduce_add(sum);
    if (lane == 0) s_w[wave] = sum;
    __syncthreads();
    uint32_t before = 0;
#pragma unroll
    for (int w = 0; w < BLK / 64; ++w) before += s_w[w];
    bool overflow = false;
    for (int tile = tile0; tile < tile1; ++tile) {          // (uniform)
        const uint32_t c = a.counts[tile];
        const int32_t lf = a.lastf[tile];
        const int64_t base = a.frame_off[a.first_slot] + before;
        if (threadIdx.x == 0 && lf >= 0) a.frame_off[a.first_slot + lf + 1] = base + c;
        const float4 *rp = a.rec_p + (size_t)tile * a.tile_points;
        const uint32_t *rc = a.rec_c + (size_t)tile * a.tile_points;
        for (uint32_t j = threadIdx.x; j < c; j += BLK) {
            float4 p;
            uint32_t col;
            if (NT) {
                typedef float f4 __attribute__((ext_vector_type(4)));
                const f4 v = __builtin_nontemporal_load(reinterpret_cast<const f4 *>(rp + j));
                p = make_float4(v.x, v.y, v.z, v.w);
                col = __builtin_nontemporal_load(rc + j);
            } else {
                p = pca_ldg4(reinterpret_cast<const float *>(rp + j));
                col = pca_ldg(rc + j);
            }
            const int64_t o = base + j;
            if (o >= a.st.capacity) { overflow = true; continue; }
            if (NT) {
                __builtin_nontemporal_store((double)p.x, a.st.x + o);
                __builtin_nontemporal_store((double)p.y, a.st.y + o);
                __builtin_nontemporal_store((double)p.z, a.st.z + o);
                __builtin_nontemporal_store(p.w, a.st.intensity + o);
                __builtin_nontemporal_store(col, a.st.rgbs + o);
                __builtin_nontemporal_store((int32_t)0, a.st.inst + o);
                __builtin_nontemporal_store((uint8_t)0, a.st.dyn + o);
            } else {
                a.st.x[o] = (double)p.x;
                a.st.y[o] = (double)p.y;
                a.st.z[o] = (double)p.z;
                a.st.intensity[o] = p.w;
                a.st.rgbs[o] = col;
                a.st.inst[o] = 0;
                a.st.dyn[o] = 0;
            }
        }
        before += c;
    }
    if (overflow) pca_raise(a.status, PCA_STATUS_STORE_OVERFLOW);
}
__global__ __launch_bounds__(K1_APPEND_BLK) void k1_append(const K1AppendArgs a) { k1_append_body<false>(a); }
__global__ __launch_bounds__(K1_APPEND_BLK) void k1_append_nt(const K1AppendArgs a) { k1_append_body<true>(a); }

// ---- host side ----
#define K1_FUSED_BLK 256        // FUSED: many small tiles (one frame = 118 workgroups), latency matters
#define K1_FUSED_PPT 4
#define K1_SPLIT_BLK 512        // SPLIT: 72 us for 64 x 120 k points (256 x 4 and 1024 x 4: 81-82)
#define K1_SPLIT_PPT 4
#define K1_SPLIT_TILE (K1_SPLIT_BLK * K1_SPLIT_PPT)
#define K1_TAIL_BLK 1024        // the deferred frame riding in level 1 of the raster (pca_k1_prepare_pending)
#define K1_TAIL_PPT 4

// The kernels the host launches, each by [bilinear]; the SPLIT front kernel also by where the descriptors travel (uploaded /
// inline in the kernel arguments), k1_append by [nt].
typedef void (*K1Kernel)(K1Args);
typedef void (*K1InlineKernel)(K1Args, K1InlineFrames);
typedef void (*K1AppendKernel)(K1AppendArgs);
static const K1Kernel g_k1_fused[2] = {k1_kitti<K1_FUSED_BLK, K1_FUSED_PPT, false, false>, k1_kitti<K1_FUSED_BLK, K1_FUSED_PPT, false, true>};
static const K1Kernel g_k1_split[2] = {k1_kitti<K1_SPLIT_BLK, K1_SPLIT_PPT, true, false>, k1_kitti<K1_SPLIT_BLK, K1_SPLIT_PPT, true, true>};
static const K1InlineKernel g_k1_split_inl[2] = {k1_kitti_inl<K1_SPLIT_BLK, K1_SPLIT_PPT, false>, k1_kitti_inl<K1_SPLIT_BLK, K1_SPLIT_PPT, true>};
static const K1AppendKernel g_k1_append[2] = {k1_append, k1_append_nt};

// Every PCA_K1_* switch (README: tuning and diagnostics; results are identical, only speed changes).
struct K1Tuning { bool force_split, no_inline, stamps, append_nt; int queues, append_group; };
static K1Tuning k1_tuning()
{
    K1Tuning t;
    // read on every call: tests and tools set them inside a running process
    t.force_split = !strcmp(pca_env_str("PCA_K1_MODE"), "split");      // the SPLIT form also where FUSED would do
    t.queues = (int)pca_env_int("PCA_K1_QUEUES", 0, 1, K1_MAXQ);       // queues of the SPLIT front kernel (0: one per frame, at most K1_MAXQ)
    t.no_inline = pca_env_int("PCA_K1_NO_INLINE", 0) != 0;             // descriptors uploaded also where they fit the kernel arguments
    t.stamps = pca_env_int("PCA_K1_STAMPS", 0) != 0;                   // in-kernel phase stamps (pca_debug_k1_stamps)
    // PCA_K1_APPEND="<group>[,nt]", read once per process (A/B): consecutive tiles per workgroup of k1_append, 1..64, and its
    // non-temporal form.  Default: one tile per workgroup (4 and 8 measured the same), plain loads and stores.  Non-temporal: the
    // kernel itself takes 23 instead of 17 us; it wins only where the NEXT call's inputs would otherwise be pushed out of the
    // Infinity Cache (64 frames cycled: 69.9 -> 60-64 us), loses on cached inputs (8 frames: 49.7 -> 54.1) and changes nothing
    // when the inputs come from HBM (two alternating batches: 75.3 / 75.4): profiles/r05_experiments/k1_round5.txt
    const int64_t group = PCA_ENV_ONCE("PCA_K1_APPEND", 1);
    static const bool nt = strstr(pca_env_str("PCA_K1_APPEND"), "nt") != nullptr;
    t.append_group = (int)(group < 1 ? 1 : group > 64 ? 64 : group); t.append_nt = nt;
    return t;
}

// What all plans of one call share.
struct K1Call { const double *P; int H, W; const uint64_t *filter_mask; const pca_store *store; int64_t *frame_off; int sample_mode; hipStream_t s; K1Tuning tune; };
// One (sub-)batch of a call: frames, first slot, its descriptors on the host (k1_assign_queues fills them) and where they are uploaded to.
struct K1Batch { const pca_kitti_frame *frames; int n_frames, first_slot; K1Frame *hf; const K1Frame *df; };
struct K1Plan {                   // the launch arguments of one (sub-)batch
    K1Args fa;
    K1AppendArgs pa;
    dim3 grid_front;              // FUSED: (tiles); SPLIT: see k1_kitti
    int tiles;
    const K1Frame *host_frames;   // the plan's descriptors on the host
    bool inline_frames;           // they fit the kernel arguments: no device copy needed
};
static inline int k1_tiles_of(int n, int tile_pts) { return n > 0 ? (n + tile_pts - 1) / tile_pts : 1; }   // (an empty frame runs one tile: it closes its segment)

// SPLIT workspace of a (sub-)batch: counts u32[tiles] | lastf i32[tiles] | rec_c u32[tiles * tile_pts] | rec_p float4[tiles * tile_pts],
// as byte offsets from the base, and its size.  The only place that knows the layout: the entry point grows ctx->k1_ws to
// `total` of the largest sub-batch, k1_plan_split places the regions.
struct K1WsLayout { int64_t counts, lastf, rec_c, rec_p, total; };
static K1WsLayout k1_ws_layout(int64_t tiles, int tile_pts)
{
    const int64_t slots = tiles * tile_pts;
    K1WsLayout l;
    l.counts = 0; l.lastf = pca_align256(tiles * 4);
    l.rec_c = pca_align256(l.lastf + tiles * 4); l.rec_p = pca_align256(l.rec_c + slots * 4);
    l.total = l.rec_p + slots * 16;
    return l;
}
// The camera block: P, the bound of the conservative test, filter, store and status word; what only one form uses starts empty.
static void k1_fill_camera(pca_ctx *ctx, const K1Call &c, int first_slot, K1Args &a)
{
    const double *P = c.P;
    for (int i = 0; i < 12; ++i) a.P.m[i] = P[i];
    a.H = c.H; a.W = c.W; a.sample_mode = c.sample_mode;
    // f32 rows and the error bound of the conservative test: 2^-19 relative is 6x the worst case of three
    // rounded coefficients and four fma roundings per form (< 2^-21.6), so a point is only ever culled when its
    // exact f64 projection is outside the frustum by a wide margin -- as long as no form overflows (cull[16] below)
    const double g = 1.0 / 524288.0;
    const double wh = (double)(c.W > c.H ? c.W : c.H) + 1.0;
    double sx = 0, sy = 0, sd = 0;
    for (int j = 0; j < 3; ++j) { sx += fabs(P[j]); sy += fabs(P[4 + j]); sd += fabs(P[8 + j]); }
    for (int i = 0; i < 12; ++i) a.cull[i] = (float)P[i];
    a.cull[12] = (float)(g * (sx + sy + wh * sd) * 1.0000002);
    a.cull[13] = (float)(g * (fabs(P[3]) + fabs(P[7]) + wh * fabs(P[11])) * 1.0000002 + 1e-30);
    a.cull[14] = (float)((double)c.W - 0.5);
    a.cull[15] = (float)((double)c.H - 0.5);
    // The bound above is one of rounding errors: it says nothing once a form or a partial sum of its chain overflows.  Each is at
    // most A max|xyz| + B in magnitude; while that stays below FLT_MAX / 4 nothing overflows (f32 roundings included).  Beyond the
    // max|xyz| of cull[16] the kernel culls nothing.
    const double A = sx + sy + wh * sd;
    const double B = fabs(P[3]) + fabs(P[7]) + wh * fabs(P[11]);
    const double lim = ((double)FLT_MAX / 4 - B) / A;              // (A = 0: +inf)
    if (!(lim > 0)) a.cull[16] = -1.0f;                            // a huge or NaN P: every max|xyz| is beyond it
    else if (lim >= (double)FLT_MAX) a.cull[16] = FLT_MAX;         // only inf is beyond it
    else a.cull[16] = nextafterf((float)lim, 0.0f);                // (rounded towards the safe side)
    for (int i = 0; i < 4; ++i) a.filt.w[i] = c.filter_mask ? c.filter_mask[i] : 0;
    a.st = *c.store; a.frame_off = c.frame_off; a.first_slot = first_slot;
    a.status = ctx->ticket + 1;
    a.state = nullptr; a.epoch = 0; a.dbg = nullptr;
    a.rec_p = nullptr; a.rec_c = nullptr; a.counts = nullptr; a.lastf = nullptr;
}
// The queue assignment, the descriptors b.hf[0..n_frames) sorted by queue, and the front grid.  SPLIT: frame f -> queue f % Q,
// block b -> position b / Q of queue b % Q (a frame's image lines stay in one L2); FUSED: Q = 1, one workgroup per tile.
static int k1_assign_queues(pca_ctx *ctx, const K1Batch &b, int tile_pts, int Q, bool fused, K1Plan *plan)
{
    K1Args &a = plan->fa;
    const int n_frames = b.n_frames;
    std::vector<int> tile0(n_frames);                       // first tile of frame k in frame order
    int total = 0;
    bool equal = true;                                      // the same number of tiles in every frame
    for (int k = 0; k < n_frames; ++k) {
        tile0[k] = total;
        total += k1_tiles_of(b.frames[k].n, tile_pts);
        equal = equal && k1_tiles_of(b.frames[k].n, tile_pts) == k1_tiles_of(b.frames[0].n, tile_pts);
    }
    int w = 0, maxq = 0, maxf = 0;
    for (int q = 0; q < K1_MAXQ; ++q) {
        a.qframe0[q] = w;
        int qpos = 0;
        if (q < Q)
            for (int k = q; k < n_frames; k += Q) {
                K1Frame &d = b.hf[w++];
                const pca_kitti_frame &f = b.frames[k];
                d.pts = f.pts; d.rgb = f.rgb; d.sem = f.sem; d.sem_gt = f.sem_gt;
                d.n = f.n; d.tile0 = tile0[k]; d.qpos0 = qpos; d.f = k;
                qpos += k1_tiles_of(f.n, tile_pts);
            }
        a.qtiles[q] = qpos;
        if (qpos > maxq) maxq = qpos;
        if (w - a.qframe0[q] > maxf) maxf = w - a.qframe0[q];
    }
    a.qframe0[K1_MAXQ] = w;
    a.n_frames = n_frames; a.n_queues = Q; a.qbase = n_frames / Q; a.qrem = n_frames % Q;
    a.tpf = equal ? k1_tiles_of(b.frames[0].n, tile_pts) : 0;
    a.frames = n_frames > 1 ? b.df : nullptr; a.one = b.hf[0];
    plan->host_frames = b.hf; plan->tiles = total;
    plan->grid_front = fused ? dim3(total) : a.tpf ? dim3(Q, a.tpf, maxf) : dim3(Q, maxq);
    if (!fused && (maxq > 65535 || maxf > 65535)) { ctx->err = "k1: batch too large"; return -1; }
    return 0;
}
// PCA_K1_STAMPS: the stamp buffer (8 words per workgroup of the front grid), cleared for this launch
static int k1_arm_stamps(pca_ctx *ctx, K1Plan *plan, hipStream_t s)
{
    const int64_t nblocks = (int64_t)plan->grid_front.x * plan->grid_front.y * plan->grid_front.z;
    if (!ctx->dbg) PCA_CHECK(ctx, hipMalloc(&ctx->dbg, sizeof(unsigned long long) * 8 * 65536));
    if (nblocks <= 65536) { plan->fa.dbg = ctx->dbg; PCA_CHECK(ctx, hipMemsetAsync(ctx->dbg, 0, sizeof(unsigned long long) * 8 * nblocks, s)); }
    ctx->dbg_blocks = (int)(nblocks < 65536 ? nblocks : 65536);
    return 0;
}
// FUSED: one launch of `tile_pts`-point tiles chained by look-back -- its state reserved, its epoch drawn
static int k1_plan_fused(pca_ctx *ctx, const K1Call &c, const K1Batch &b, int tile_pts, K1Plan *plan)
{
    k1_fill_camera(ctx, c, b.first_slot, plan->fa);
    if (k1_assign_queues(ctx, b, tile_pts, 1, true, plan)) return -1;
    plan->inline_frames = false;
    if (c.tune.stamps && k1_arm_stamps(ctx, plan, c.s)) return -1;
    if (pca_ctx_reserve_tiles(ctx, plan->tiles, c.s)) return -1;
    plan->fa.state = ctx->tile_state;
    plan->fa.epoch = pca_ctx_next_epoch(ctx, c.s);
    return 0;
}
// SPLIT: front kernel + k1_append over the workspace (grown by the caller BEFORE any plan is made: the plans hold pointers into it)
static int k1_plan_split(pca_ctx *ctx, const K1Call &c, const K1Batch &b, K1Plan *plan)
{
    K1Args &a = plan->fa;
    int Q = b.n_frames < K1_MAXQ ? b.n_frames : K1_MAXQ;
    if (c.tune.queues) Q = c.tune.queues < b.n_frames ? c.tune.queues : b.n_frames;
    k1_fill_camera(ctx, c, b.first_slot, a);
    if (k1_assign_queues(ctx, b, K1_SPLIT_TILE, Q, false, plan)) return -1;
    plan->inline_frames = a.tpf && b.n_frames > 1 && b.n_frames <= K1_INLINE_FRAMES && !c.tune.no_inline;
    if (c.tune.stamps && k1_arm_stamps(ctx, plan, c.s)) return -1;
    const K1WsLayout l = k1_ws_layout(plan->tiles, K1_SPLIT_TILE);
    char *ws = reinterpret_cast<char *>(ctx->k1_ws);
    a.counts = reinterpret_cast<uint32_t *>(ws + l.counts); a.lastf = reinterpret_cast<int32_t *>(ws + l.lastf);
    a.rec_c = reinterpret_cast<uint32_t *>(ws + l.rec_c); a.rec_p = reinterpret_cast<float4 *>(ws + l.rec_p);
    K1AppendArgs &pa = plan->pa;
    pa.rec_p = a.rec_p; pa.rec_c = a.rec_c; pa.counts = a.counts; pa.lastf = a.lastf;
    pa.tile_points = K1_SPLIT_TILE; pa.tiles = plan->tiles;
    pa.group = plan->tiles / c.tune.append_group >= 4 * ctx->n_cu ? c.tune.append_group : 1;     // (small batches: as many workgroups as there are tiles)
    pa.st = *c.store; pa.frame_off = c.frame_off; pa.first_slot = b.first_slot; pa.status = a.status;
    return 0;
}
static int k1_launch(pca_ctx *ctx, const K1Call &c, const K1Plan *plan, bool fused)
{
    hipStream_t s = c.s;
    const int bilin = plan->fa.sample_mode != 0;
    if (fused) {
        hipLaunchKernelGGL(g_k1_fused[bilin], plan->grid_front, dim3(K1_FUSED_BLK), 0, s, plan->fa);
    } else {
        K1InlineFrames inl;
        if (plan->inline_frames) memcpy(inl.f, plan->host_frames, sizeof(K1Frame) * plan->fa.n_frames);
        if (plan->inline_frames) hipLaunchKernelGGL(g_k1_split_inl[bilin], plan->grid_front, dim3(K1_SPLIT_BLK), 0, s, plan->fa, inl);
        else hipLaunchKernelGGL(g_k1_split[bilin], plan->grid_front, dim3(K1_SPLIT_BLK), 0, s, plan->fa);
        const dim3 agrid((plan->tiles + plan->pa.group - 1) / plan->pa.group);
        hipLaunchKernelGGL(g_k1_append[c.tune.append_nt], agrid, dim3(K1_APPEND_BLK), 0, s, plan->pa);
    }
    PCA_CHECK(ctx, hipGetLastError());
    return 0;
}

// ---- the steps of pca_kitti_project_sample_filter_ex ----
// K1's checks of a call's frames, the ONE place that knows them: pca_kitti_project_sample_filter_ex runs them before it plans,
// pca_kitti_integrate before it stages, notes (pca_k1_defer) or steps anything -- a noted frame goes to the GPU unchecked
// (pca_k1_prepare_pending).
int pca_k1_check_frames(pca_ctx *ctx, const pca_kitti_frame *frames, int n_frames, const double *P, int H, int W,
                        const pca_store *store, const int64_t *frame_off, int sample_mode)
{
    if (sample_mode != PCA_SAMPLE_NEAREST && sample_mode != PCA_SAMPLE_BILINEAR) { ctx->err = "k1: unknown sample_mode"; return -1; }
    if (!frames || n_frames <= 0 || !store || !frame_off || !P) { ctx->err = "k1: bad arguments"; return -1; }
    if (H < 0 || W < 0) { ctx->err = "k1: H and W must not be negative"; return -1; }
    if ((int64_t)H * W * 3 >= (1ll << 31)) { ctx->err = "k1: image too large"; return -1; }
    for (int k = 0; k < n_frames; ++k) {
        const pca_kitti_frame &f = frames[k];
        if (f.n < 0 || (f.n > 0 && !f.pts)) { ctx->err = "k1: bad frame (n < 0, or points without pts)"; return -1; }
        if (!f.sem_gt && f.n > 0 && (!f.rgb || !f.sem || (int64_t)H * W == 0)) { ctx->err = "k1: frame needs rgb+sem or sem_gt"; return -1; }
    }
    return 0;
}
static int k1_validate(pca_ctx *ctx, const K1Call &c, const pca_kitti_frame *frames, int n_frames)
{
    return pca_k1_check_frames(ctx, frames, n_frames, c.P, c.H, c.W, c.store, c.frame_off, c.sample_mode);
}
// The colour gather is one 4-byte load per point: a one-pixel image (3 bytes) is handed to the kernel as a 4-byte copy (*frames: then `padded`)
static int k1_pad_tiny_images(pca_ctx *ctx, const K1Call &c, const pca_kitti_frame **frames, int n_frames, std::vector<pca_kitti_frame> *padded)
{
    const pca_kitti_frame *in = *frames;
    if (c.H * c.W * 3 >= 4 || c.H * c.W == 0) return 0;
    bool any = false;
    for (int k = 0; k < n_frames; ++k) any = any || (in[k].rgb && !in[k].sem_gt);
    if (!any) return 0;
    if (pca_dev_grow(ctx, &ctx->k1_tiny, &ctx->k1_tiny_cap, (int64_t)n_frames * 4, c.s)) return -1;
    PCA_CHECK(ctx, hipMemsetAsync(ctx->k1_tiny, 0, (size_t)n_frames * 4, c.s));
    padded->assign(in, in + n_frames);
    for (int k = 0; k < n_frames; ++k)
        if (in[k].rgb && !in[k].sem_gt) {
            uint8_t *dst = reinterpret_cast<uint8_t *>(ctx->k1_tiny) + 4 * k;
            PCA_CHECK(ctx, hipMemcpyAsync(dst, in[k].rgb, (size_t)c.H * c.W * 3, hipMemcpyDeviceToDevice, c.s));
            (*padded)[k].rgb = dst;
        }
    *frames = padded->data();
    return 0;
}
// Frame descriptors of the whole call: built in pinned memory (two blocks, alternating between calls), one asynchronous
// upload.  *pin_slot: the pinned block to use, ctx->k1_pin[*pin_slot] -- free by now, room for n_frames; room on the device too.
static int k1_stage_descriptors(pca_ctx *ctx, int n_frames, hipStream_t s, int *pin_slot)
{
    const int slot = *pin_slot = ctx->k1_pin_next;
    ctx->k1_pin_next ^= 1;
    if (ctx->k1_pin_busy[slot]) { PCA_CHECK(ctx, hipEventSynchronize(ctx->k1_pin_ev[slot])); ctx->k1_pin_busy[slot] = false; }
    if (n_frames > ctx->k1_pin_cap[slot]) {
        if (ctx->k1_pin[slot]) PCA_CHECK(ctx, hipHostFree(ctx->k1_pin[slot]));
        ctx->k1_pin[slot] = nullptr; ctx->k1_pin_cap[slot] = 0;
        PCA_CHECK(ctx, hipHostMalloc(reinterpret_cast<void **>(&ctx->k1_pin[slot]), sizeof(K1Frame) * (size_t)n_frames * 2, hipHostMallocMapped));
        ctx->k1_pin_cap[slot] = n_frames * 2;
    }
    if (!ctx->k1_pin_ev[slot]) PCA_CHECK(ctx, hipEventCreateWithFlags(&ctx->k1_pin_ev[slot], hipEventDisableTiming));
    return pca_dev_grow(ctx, &ctx->k1_frames_dev, &ctx->k1_frames_cap, (int64_t)sizeof(K1Frame) * n_frames, s);
}
// (fetched by a kernel from the mapped host block: a copy command of a few KB costs 13-17 us, see pca_fetch_block)
static int k1_upload_descriptors(pca_ctx *ctx, int pin_slot, int n_frames, hipStream_t s)
{
    if (pca_fetch_block(ctx, ctx->k1_pin[pin_slot], 0, ctx->k1_frames_dev, (int64_t)sizeof(K1Frame) * n_frames, s)) return -1;
    PCA_CHECK(ctx, hipEventRecord(ctx->k1_pin_ev[pin_slot], s));
    ctx->k1_pin_busy[pin_slot] = true;
    return 0;
}
// SPLIT: the call as sub-batches of at most K1_MAX_SPLIT_TILES tiles (k1_append adds up the counts before its tile), taken
// greedily, at least one frame each: sub-batch i = frames [cuts[i], cuts[i + 1]).  *max_tiles: the tiles of the largest.
static int k1_cut_batches(pca_ctx *ctx, const pca_kitti_frame *frames, int n_frames, std::vector<int> *cuts, int64_t *max_tiles)
{
    auto tiles = [&](int k) { return (int64_t)k1_tiles_of(frames[k].n, K1_SPLIT_TILE); };
    cuts->assign(1, 0); *max_tiles = 0;
    for (int k0 = 0, k1; k0 < n_frames; k0 = k1) {
        int64_t t = tiles(k0);
        if (t > (1 << 28)) { ctx->err = "k1: frame too large"; return -1; }
        for (k1 = k0 + 1; k1 < n_frames && t + tiles(k1) <= K1_MAX_SPLIT_TILES; ++k1) t += tiles(k1);
        if (t > *max_tiles) *max_tiles = t;
        cuts->push_back(k1);
    }
    return 0;
}

// ---- deferred K1 (pca_common.h: K1Pending) ----
// the staging block of pca_kitti_integrate is free again once the K1 launched on `s` has read it
static void k1_release_stage(pca_ctx *ctx, int stage_idx, hipStream_t s)
{
    if (stage_idx < 0) return;
    pca_ctx::Stage &st = ctx->stage[stage_idx];
    if (hipEventRecord(st.done, s) == hipSuccess) st.busy = true;
    else (void)hipStreamSynchronize(s);
}
int pca_k1_flush_pending(pca_ctx *ctx)
{
    if (!ctx || !ctx->k1_pend.valid) return 0;
    pca_ctx::K1Pending pd = ctx->k1_pend;
    ctx->k1_pend.valid = false;                             // (first: the call below comes back through here)
    const int rc = pca_kitti_project_sample_filter_ex(ctx, &pd.fr, 1, pd.P, pd.H, pd.W, pd.filt, &pd.store, pd.frame_off, pd.slot,
                                                      pd.sample_mode, pd.stream);
    k1_release_stage(ctx, pd.stage_idx, pd.stream);
    return rc;
}
// The deferred frame as level 1 of the raster takes it: the argument block of a FUSED launch with 1024 x 4 tiles (look-back
// state reserved, epoch drawn).  *n_tiles = its workgroups.  The caller launches, then calls pca_k1_pending_launched.
int pca_k1_prepare_pending(pca_ctx *ctx, K1Args *out, int *n_tiles, hipStream_t s)
{
    pca_ctx::K1Pending &pd = ctx->k1_pend;
    if (!pd.valid) return -1;
    const K1Call c = {pd.P, pd.H, pd.W, pd.filt, &pd.store, pd.frame_off, pd.sample_mode, s, k1_tuning()};
    K1Frame hf;
    K1Plan plan;
    const K1Batch b = {&pd.fr, 1, pd.slot, &hf, nullptr};
    if (k1_plan_fused(ctx, c, b, K1_TAIL_BLK * K1_TAIL_PPT, &plan)) return -1;
    *out = plan.fa; *n_tiles = plan.tiles;
    return 0;
}
void pca_k1_pending_launched(pca_ctx *ctx, hipStream_t s)
{
    k1_release_stage(ctx, ctx->k1_pend.stage_idx, s);
    ctx->k1_pend.valid = false;
}

// ---- C ABI ----
extern "C" {

// diagnostic: copies the stamps of the last K1 launch (8 words per workgroup) to `out`; returns the workgroup count
int pca_debug_k1_stamps(pca_ctx *ctx, unsigned long long *out, int max_blocks)
{
    if (!ctx || !ctx->dbg) return 0;
    const int n = ctx->dbg_blocks < max_blocks ? ctx->dbg_blocks : max_blocks;
    if (hipMemcpy(out, ctx->dbg, sizeof(unsigned long long) * 8 * n, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return n;
}

// K1 of pca_kitti_integrate deferred into the next raster of this context (see pca.h); on = 0 also runs what is pending.
int pca_k1_defer(pca_ctx *ctx, int on)
{
    if (!ctx) return -1;
    ctx->k1_defer = on != 0;
    return on ? 0 : pca_k1_flush_pending(ctx);
}
int pca_k1_flush(pca_ctx *ctx) { return ctx ? pca_k1_flush_pending(ctx) : -1; }

int pca_kitti_project_sample_filter(pca_ctx *ctx, const pca_kitti_frame *frames, int n_frames, const double P[12],
                                    int H, int W, const uint64_t filter_mask[4], const pca_store *store,
                                    int64_t *frame_off, int first_slot, void *stream)
{
    return pca_kitti_project_sample_filter_ex(ctx, frames, n_frames, P, H, W, filter_mask, store, frame_off, first_slot,
                                              PCA_SAMPLE_NEAREST, stream);
}

int pca_kitti_project_sample_filter_ex(pca_ctx *ctx, const pca_kitti_frame *frames, int n_frames, const double P[12],
                                       int H, int W, const uint64_t filter_mask[4], const pca_store *store,
                                       int64_t *frame_off, int first_slot, int sample_mode, void *stream)
{
    if (!ctx) return -1;
    if (pca_k1_flush_pending(ctx)) return -1;               // (an earlier frame whose K1 was deferred: it comes first)
    hipStream_t s = (hipStream_t)stream;
    const K1Call c = {P, H, W, filter_mask, store, frame_off, sample_mode, s, k1_tuning()};
    if (k1_validate(ctx, c, frames, n_frames)) return -1;
    PCA_CHECK(ctx, hipSetDevice(ctx->device));
    std::vector<pca_kitti_frame> padded;
    if (k1_pad_tiny_images(ctx, c, &frames, n_frames, &padded)) return -1;
    // FUSED when every workgroup of the launch is resident at once (one tile per CU at most), else SPLIT
    int64_t fused_tiles = 0;
    for (int k = 0; k < n_frames; ++k) fused_tiles += k1_tiles_of(frames[k].n, K1_FUSED_BLK * K1_FUSED_PPT);
    const bool fused = fused_tiles <= ctx->n_cu && !c.tune.force_split;
    int pin_slot;
    if (k1_stage_descriptors(ctx, n_frames, s, &pin_slot)) return -1;
    K1Frame *hf = ctx->k1_pin[pin_slot];
    const K1Frame *df = reinterpret_cast<const K1Frame *>(ctx->k1_frames_dev);
    // plan: FUSED one launch; SPLIT the sub-batches, which run one after the other on the stream and share ONE workspace --
    // grown once, for the largest of them, before any plan takes pointers into it
    std::vector<int> cuts = {0, n_frames};
    if (!fused) {
        int64_t max_tiles;
        if (k1_cut_batches(ctx, frames, n_frames, &cuts, &max_tiles)) return -1;
        if (pca_dev_grow(ctx, &ctx->k1_ws, &ctx->k1_ws_cap, k1_ws_layout(max_tiles, K1_SPLIT_TILE).total, s)) return -1;
    }
    std::vector<K1Plan> plans(cuts.size() - 1);
    bool need_upload = false;
    for (size_t i = 0; i < plans.size(); ++i) {
        const int k0 = cuts[i];
        const K1Batch b = {frames + k0, cuts[i + 1] - k0, first_slot + k0, hf + k0, df + k0};
        if (fused ? k1_plan_fused(ctx, c, b, K1_FUSED_BLK * K1_FUSED_PPT, &plans[i]) : k1_plan_split(ctx, c, b, &plans[i])) return -1;
        need_upload = need_upload || (plans[i].fa.frames && !plans[i].inline_frames);
    }
    if (ctx->profiling == 1) pca_prof_begin(ctx, PCA_K_KITTI, s);      // one event pair around the unit's GPU work
    int rc = need_upload ? k1_upload_descriptors(ctx, pin_slot, n_frames, s) : 0;
    for (size_t i = 0; i < plans.size() && rc == 0; ++i) rc = k1_launch(ctx, c, &plans[i], fused);
    if (ctx->profiling == 1) pca_prof_end(ctx, s);
    return rc;
}

}  // extern "C"
