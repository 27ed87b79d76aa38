// pca_bev_elev.hip -- the BEV window partitioned by height above the cell minimum: two passes over the window for gfx950.
//
// The reference's SemBEVGenerator.static_obj_partitioning_by_elev (bev_generator/sem_bev.py:556-591) builds the per-cell
// minimum-z map of the rows it is given and flags every row whose z lies more than elev_thresh above its cell's minimum: two
// per-point Python loops.  Here pass one is a cell minimum and pass two compares each point with its cell, on the two-level
// scaffold of pca_bev_side.h (LDS atomics only, no global atomics); the view test, the cell and the owed re-transforms are
// pca_bev_view.h's.
//
//   level 1  bev_elev_bin      side_bin with key = tile << 6 | cell_in_tile; the kept points' records are {z in the BEV frame
//                              f64, index in the window u32, cell_in_tile u32}, 16 bytes.  A point that is NOT kept gets
//                              flags[index] = 255 here (coalesced).  Key and z stay in registers between the passes.
//   level 2  bev_elev_cells    side_tile_runs / side_find; pass A: LDS minimum per cell over the order-preserving u64 key of z
//                              (the main raster's elevation plane), barrier, pass B: elevated = z > (min + elev_thresh) as an
//                              f64 add and an f64 compare, flags[index] = elevated; counts per tile in LDS; whole tile rows of
//                              `elev` and `observed`; three int64 words per tile for the totals.
//   tail     bev_elev_totals   one workgroup: the per-tile words summed into counts[3] (no global atomics).
// Every byte of flags[0, n) is written exactly once per call: by level 1 (255) or by level 2 (0 / 1).
// The order in which a tile's records arrive is not fixed (LDS cursors); neither the minimum nor a flag depends on it.
#include "pca_bev_common.h"
#include "pca_bev_side.h"

#define EB_REG_P 12               // points per thread of level 1 whose key and z stay in registers between its passes
#define EC_THREADS SIDE_CELLS_THREADS
#define ET_THREADS 1024           // workgroup size of the tail

struct alignas(16) ElvRec { double z; uint32_t idx, cell; };

struct alignas(16) ElvArgs {
    SideArgs s;                   // (slot_split = slot_begin: the partition knows no sets)
    double thresh;
    int include_dyn;
    ElvRec *recs;                 // [max_points + G], tile-ordered per segment
    int64_t *tile_counts;         // [3][T]: in view, elevated, not elevated
    double *elev;                 // [px][px] or NULL
    uint8_t *observed;            // [px][px] or NULL
    uint8_t *flags;               // [window points] or NULL
    int64_t *counts;              // [3] or NULL
};

// ---------------------------------------------------------------------------------------------
// level 1
// ---------------------------------------------------------------------------------------------
struct ElvBin {
    static constexpr int REG_P = EB_REG_P, SHIFT = 6;
    struct Payload { double z = 0.0; };                     // the point's height in the BEV frame
    ElvRec *recs;
    uint8_t *flags;
    bool all_dyn;
    // key of stored point p: the view's key (tile << 7 | cell_in_tile << 1 | set, set = 0) >> 1
    __device__ __forceinline__ uint32_t key(const SideArgs &a, const ViewConst &vc, const PendHi &pend_hi, const SideWindow &, int64_t p, Payload &pl) const
    {
        double X = pca_ldg(a.st.x + p), Y = pca_ldg(a.st.y + p), Z = pca_ldg(a.st.z + p);
        const uint8_t D = pca_ldg(a.st.dyn + p);
        apply_owed(a.owed, pend_hi, p, X, Y, Z);
        pl.z = (Z - vc.oz) + 0.0;                           // (the reference's matmul turns a z of -0.0 into +0.0)
        const uint32_t vk = view_key_lean<false>(vc, X, Y, Z, all_dyn || D != 1, 0u);
        return vk == KEY_INVALID ? KEY_INVALID : vk >> 1;
    }
    __device__ __forceinline__ void dropped(const SideWindow &w, int64_t p) const { if (flags) flags[p - w.lo] = 255; }
    __device__ __forceinline__ void store(int g, const SideWindow &w, uint32_t pos, uint32_t key, const Payload &pl, int64_t p) const
    {
        const uint64_t zb = (uint64_t)__double_as_longlong(pl.z);
        *reinterpret_cast<uint4 *>(recs + ((int64_t)g * w.chunk + pos)) =
            make_uint4((uint32_t)zb, (uint32_t)(zb >> 32), (uint32_t)(p - w.lo), key & 63u);   // one 16-byte store
    }
};
__global__ __launch_bounds__(SIDE_BIN_THREADS) void bev_elev_bin(const ElvArgs a) { side_bin(a.s, ElvBin{a.recs, a.flags, a.include_dyn != 0}); }

// ---------------------------------------------------------------------------------------------
// level 2
// ---------------------------------------------------------------------------------------------
// the r-th record of the tile
__device__ __forceinline__ uint4 elv_load_rec(const ElvArgs &a, const uint32_t *s_pre, const uint32_t *s_off, int places, uint32_t r)
{
    const int lo = side_find(s_pre, places, r);
    return *reinterpret_cast<const uint4 *>(a.recs + ((size_t)s_off[lo] + (r - s_pre[lo])));
}
__global__ __launch_bounds__(EC_THREADS) void bev_elev_cells(const ElvArgs a)
{
    __shared__ unsigned long long s_min[TCELLS];            // order key of the cell's minimum z, ~0 = no record
    __shared__ uint32_t s_pre[SIDE_PLACES + 1], s_off[SIDE_PLACES], s_wsum[EC_THREADS / 64];   // side_tile_runs
    __shared__ uint32_t s_elevated;
    const int tile = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (tid < TCELLS) s_min[tid] = ~0ull;
    if (tid == 0) s_elevated = 0;
    int places;
    const uint32_t total = side_tile_runs(a.s, tile, s_pre, s_off, s_wsum, places);
    // pass A: the minimum per cell (a record that cannot lower what the cell holds by now skips the atomic)
    for (uint32_t r = tid; r < total; r += EC_THREADS) {
        const uint4 rec = elv_load_rec(a, s_pre, s_off, places, r);
        const uint64_t zb = ((uint64_t)rec.y << 32) | rec.x;
        const unsigned long long key = f64_order_key(__longlong_as_double((long long)zb));
        if (key < *(volatile unsigned long long *)&s_min[rec.w]) atomicMin(&s_min[rec.w], key);
    }
    __syncthreads();
    // pass B: every record against its cell's minimum -- an f64 add and an f64 compare, nothing fused
    uint32_t n_elev = 0;
    for (uint32_t r = tid; r < total; r += EC_THREADS) {
        const uint4 rec = elv_load_rec(a, s_pre, s_off, places, r);
        const uint64_t zb = ((uint64_t)rec.y << 32) | rec.x;
        const double z = __longlong_as_double((long long)zb);
        const double bound = f64_from_order_key(s_min[rec.w]) + a.thresh;
        const bool elevated = z > bound;
        n_elev += elevated ? 1u : 0u;
        if (a.flags) a.flags[rec.z] = elevated ? 1 : 0;
    }
    n_elev = wave_reduce_add(n_elev);
    if ((tid & 63) == 0 && n_elev) atomicAdd(&s_elevated, n_elev);
    __syncthreads();
    // whole tile rows: eight lanes write one row of the tile
    const int px = a.s.prm.px;
    const int row0 = (tile / a.s.tx) * TS, col0 = (tile % a.s.tx) * TS;
    if (tid < TCELLS) {
        const int row = row0 + (tid >> 3), col = col0 + (tid & 7);
        if (row < px && col < px) {
            const unsigned long long k = s_min[tid];
            const bool seen = k != ~0ull;
            const size_t at = (size_t)row * px + col;
            if (a.elev) a.elev[at] = seen ? f64_from_order_key(k) : 0.0;
            if (a.observed) a.observed[at] = seen ? 1 : 0;
        }
    }
    if (tid == 0) {
        const int64_t e = (int64_t)s_elevated;
        a.tile_counts[tile] = (int64_t)total;
        a.tile_counts[(size_t)a.s.T + tile] = e;
        a.tile_counts[2 * (size_t)a.s.T + tile] = (int64_t)total - e;
    }
}

// ---------------------------------------------------------------------------------------------
// tail: the totals
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ET_THREADS) void bev_elev_totals(const ElvArgs a)
{
    __shared__ unsigned long long s_sum[3][ET_THREADS];
    const int tid = (int)threadIdx.x;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        unsigned long long v = 0;
        for (int t = tid; t < a.s.T; t += ET_THREADS) v += (unsigned long long)a.tile_counts[(size_t)q * a.s.T + t];
        s_sum[q][tid] = v;
    }
    __syncthreads();
    for (int half = ET_THREADS / 2; half > 0; half >>= 1) {
        if (tid < half) {
#pragma unroll
            for (int q = 0; q < 3; ++q) s_sum[q][tid] += s_sum[q][tid + half];
        }
        __syncthreads();
    }
    if (tid < 3) a.counts[tid] = (int64_t)s_sum[tid][0];
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
// the workspace: the records, then the table, then the per-tile totals (side_layout: `tail`)
static SideLayout elv_layout(int64_t max_points, int px) { return side_layout(max_points, px, sizeof(ElvRec), 3 * 8, "PCA_BEV_ELEV_G"); }
static const WindowPass ELV_PASS = {"bev elev partition", false, false};

extern "C" {

int64_t pca_bev_elev_workspace_bytes(int64_t max_points, int px) { return elv_layout(max_points, px).total; }

int pca_bev_elev_partition(pca_ctx *ctx, const pca_store *store, const int64_t *frame_off, int slot_begin, int slot_end,
                           int64_t max_points, const pca_bev_params *prm, double elev_thresh, int include_dyn,
                           const double *pending_Ts, const int *pending_slot_ends, int n_pending, void *workspace,
                           int64_t workspace_bytes, double *elev, uint8_t *observed, uint8_t *flags, int64_t *counts,
                           void *stream)
{
    if (!ctx) return -1;
    if (max_points < 1) max_points = 1;
    hipStream_t s = (hipStream_t)stream;
    // every check comes before the first launch (a noted K1 included)
    ElvArgs A;
    char *w;
    if (window_check(ctx, ELV_PASS, workspace && (elev || observed || flags || counts), store, frame_off, slot_begin, slot_begin,
                     slot_end, max_points, prm, pending_Ts, pending_slot_ends, n_pending, A.s))
        return -1;
    if (elev_thresh != elev_thresh) { ctx->err = "bev elev partition: elev_thresh is NaN"; return -1; }
    const SideLayout l = elv_layout(max_points, prm->px);
    if (side_tiles(ctx, ELV_PASS.what, slot_begin, workspace, workspace_bytes, l, A.s, w)) return -1;
    A.thresh = elev_thresh;
    A.include_dyn = include_dyn;
    A.recs = reinterpret_cast<ElvRec *>(w);
    A.tile_counts = reinterpret_cast<int64_t *>(w + l.tail);
    A.elev = elev; A.observed = observed; A.flags = flags; A.counts = counts;
    const ElvArgs &args = A;
    if (side_launch_bin<bev_elev_bin>(ctx, PCA_K_BEV_ELEV_BIN, args, s)) return -1;
    PCA_LAUNCH(ctx, PCA_K_BEV_ELEV_CELLS, bev_elev_cells, dim3(args.s.T), dim3(EC_THREADS), s, args);
    if (args.counts) PCA_LAUNCH(ctx, PCA_K_BEV_ELEV_CELLS, bev_elev_totals, dim3(1), dim3(ET_THREADS), s, args);
    PCA_CHECK(ctx, hipGetLastError());
    return 0;
}

}  // extern "C"
