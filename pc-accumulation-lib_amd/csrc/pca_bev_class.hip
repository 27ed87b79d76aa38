// pca_bev_class.hip -- BEV planes of any semantic class group: a counts-only pass over the window for gfx950.
//
// The main rasteriser (pca_bev.hip) turns two class sets into planes, `road` and the vehicle set, next to exact medians,
// minimum z and intensity sums.  A class plane needs none of those: per (cell, set) the number of static points and, per
// group, the number of them whose class is in the group.  This file counts ALL groups in one pass that reads 29 bytes per
// stored point (x, y, z, dyn and -- for the points inside the view -- the class byte inside rgbs), with the rasteriser's
// structure: two levels, LDS atomics only, no global atomics (a one-dword-per-lane scatter of global atomics runs at the
// memory side on this part, an order of magnitude below the streaming rate).  The two levels' scaffold is pca_bev_side.h,
// the view test, the cell and the owed re-transforms are pca_bev_view.h's.
//
//   level 1  bev_class_bin     side_bin with key = tile << 15 | cell_in_tile << 9 | set << 8 | class; the kept points' low 15
//                              key bits are the record, one uint16_t.
//   level 2  bev_class_cells   side_tile_runs / side_find, counts into LDS u32 [64 cells][2 sets][n_groups + 1] through the table
//                              class -> bit set of its groups (groups may overlap; the last slot counts every static point),
//                              closed form per (cell, set, group), whole tile rows written.
// The order in which a tile's records arrive is not fixed (LDS cursors); counts do not depend on it.
#include "pca_bev_side.h"

#define CB_REG_P 12               // points per thread of level 1 whose key stays in registers between its passes
#define CC_THREADS SIDE_CELLS_THREADS
#define CC_MAX_S (PCA_BEV_MAX_CLASS_GROUPS + 1)   // counters per (cell, set)

struct alignas(16) ClsArgs {
    SideArgs s;
    int n_groups;
    uint16_t *recs;               // [max_points + G]: cell_in_tile << 9 | set << 8 | class, tile-ordered per segment
    double *prob;                 // [3][n_groups][px][px] or NULL
    uint16_t *prob_f16;           // the same as f16 bits or NULL
    uint32_t *counts;             // [3][n_groups + 1][px][px] or NULL
    uint32_t cls_bits[256];       // class -> bit g: the class is in group g; bit n_groups: always (every static point)
};

// ---------------------------------------------------------------------------------------------
// level 1
// ---------------------------------------------------------------------------------------------
struct ClsBin {
    static constexpr int REG_P = CB_REG_P, SHIFT = 15;
    struct Payload {};
    uint16_t *recs;
    // key of stored point p: the view's key (tile << 7 | cell_in_tile << 1 | set) << 8 | class
    __device__ __forceinline__ uint32_t key(const SideArgs &a, const ViewConst &vc, const PendHi &pend_hi, const SideWindow &w, int64_t p, Payload &) const
    {
        double X = pca_ldg(a.st.x + p), Y = pca_ldg(a.st.y + p), Z = pca_ldg(a.st.z + p);
        const uint8_t D = pca_ldg(a.st.dyn + p);
        apply_owed(a.owed, pend_hi, p, X, Y, Z);
        const uint32_t vk = view_key_lean<false>(vc, X, Y, Z, D != 1, p >= w.sp ? 1u : 0u);
        if (vk == KEY_INVALID) return KEY_INVALID;
        return (vk << 8) | (pca_ldg(a.st.rgbs + p) >> 24);  // (the class byte: read for the kept points only)
    }
    __device__ __forceinline__ void dropped(const SideWindow &, int64_t) const {}
    __device__ __forceinline__ void store(int g, const SideWindow &w, uint32_t pos, uint32_t key, const Payload &, int64_t) const
    {
        recs[(int64_t)g * w.chunk + pos] = (uint16_t)(key & 0x7fffu);
    }
};
__global__ __launch_bounds__(SIDE_BIN_THREADS) void bev_class_bin(const ClsArgs a) { side_bin(a.s, ClsBin{a.recs}); }

// ---------------------------------------------------------------------------------------------
// level 2
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CC_THREADS) void bev_class_cells(const ClsArgs a)
{
    __shared__ uint32_t s_cnt[2 * TCELLS * CC_MAX_S];       // [cell][set][group | all]
    __shared__ uint32_t s_bits[256];
    __shared__ uint32_t s_pre[SIDE_PLACES + 1], s_off[SIDE_PLACES], s_wsum[CC_THREADS / 64];   // side_tile_runs
    const int tile = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int S = a.n_groups + 1;
    for (int i = tid; i < 2 * TCELLS * S; i += CC_THREADS) s_cnt[i] = 0;
    s_bits[tid] = a.cls_bits[tid];
    int places;
    const uint32_t total = side_tile_runs(a.s, tile, s_pre, s_off, s_wsum, places);
    // the tile's records: place by binary search over the prefix table, then one LDS atomic per group the class is in
    for (uint32_t r = tid; r < total; r += CC_THREADS) {
        const int lo = side_find(s_pre, places, r);
        const uint32_t rec = a.recs[(size_t)s_off[lo] + (r - s_pre[lo])];
        uint32_t bits = s_bits[rec & 255u];
        uint32_t *c = s_cnt + (rec >> 8) * S;               // (rec >> 8 = cell * 2 + set)
        while (bits) {
            atomicAdd(&c[__ffs((int)bits) - 1], 1u);
            bits &= bits - 1;
        }
    }
    __syncthreads();
    // closed forms: item = (set, group | all, cell), the cell fastest -- eight lanes write one row of the tile
    const int px = a.s.prm.px, ng = a.n_groups;
    const int row0 = (tile / a.s.tx) * TS, col0 = (tile % a.s.tx) * TS;
    const size_t plane = (size_t)px * px;
    for (int i = tid; i < 3 * S * TCELLS; i += CC_THREADS) {
        const int cell = i & 63, q = i >> 6, s = q / S, gi = q - s * S;
        const int row = row0 + (cell >> 3), col = col0 + (cell & 7);
        if (row >= px || col >= px) continue;
        const uint32_t *c0 = s_cnt + (cell * 2) * S, *c1 = c0 + S;
        const uint32_t n = s == 0 ? c0[ng] : s == 1 ? c1[ng] : c0[ng] + c1[ng];
        const size_t at = (size_t)row * px + col;
        if (gi == ng) {
            if (a.counts) a.counts[(size_t)(s * S + ng) * plane + at] = n;
            continue;
        }
        const uint32_t n_g = s == 0 ? c0[gi] : s == 1 ? c1[gi] : c0[gi] + c1[gi];
        if (a.counts) a.counts[(size_t)(s * S + gi) * plane + at] = n_g;
        // dirichlet expectation of {in the group, not in the group} with a uniform prior: finalize_cell's `dynamic` expression
        const double a_all = (double)n, a_g = (double)n_g;
        const double p = (a_g + 1.0) / ((a_g + 1.0) + ((a_all - a_g) + 1.0));
        if (a.prob) a.prob[(size_t)(s * ng + gi) * plane + at] = p;
        if (a.prob_f16) a.prob_f16[(size_t)(s * ng + gi) * plane + at] = f64_to_f16_bits(p);
    }
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
// the workspace: the uint16_t records, then the table (side_layout)
static SideLayout cls_layout(int64_t max_points, int px) { return side_layout(max_points, px, 2, 0, "PCA_BEV_CLASS_G"); }
static const WindowPass CLS_PASS = {"bev class planes", true, true};

extern "C" {

int64_t pca_bev_class_workspace_bytes(int64_t max_points, int px) { return cls_layout(max_points, px).total; }

int pca_bev_class_planes(pca_ctx *ctx, const pca_store *store, const int64_t *frame_off, int slot_begin, int slot_split,
                         int slot_end, int64_t max_points, const pca_bev_params *prm, const pca_class_group *groups,
                         int n_groups, const double *pending_Ts, const int *pending_slot_ends, int n_pending,
                         void *workspace, int64_t workspace_bytes, double *prob, uint16_t *prob_f16, uint32_t *counts,
                         void *stream)
{
    if (!ctx) return -1;
    if (max_points < 1) max_points = 1;
    hipStream_t s = (hipStream_t)stream;
    // every check comes before the first launch (a noted K1 included)
    ClsArgs A;
    char *w;
    if (window_check(ctx, CLS_PASS, groups && workspace && (prob || prob_f16 || counts), store, frame_off, slot_begin, slot_split,
                     slot_end, max_points, prm, pending_Ts, pending_slot_ends, n_pending, A.s))
        return -1;
    if (n_groups < 1 || n_groups > PCA_BEV_MAX_CLASS_GROUPS) { ctx->err = "bev class planes: n_groups must be in 1..16"; return -1; }
    if (side_tiles(ctx, CLS_PASS.what, slot_split, workspace, workspace_bytes, cls_layout(max_points, prm->px), A.s, w)) return -1;
    A.n_groups = n_groups;
    A.recs = reinterpret_cast<uint16_t *>(w);
    A.prob = prob; A.prob_f16 = prob_f16; A.counts = counts;
    for (int c = 0; c < 256; ++c) {
        uint32_t bits = 1u << n_groups;
        for (int g = 0; g < n_groups; ++g) bits |= (uint32_t)((groups[g].mask[c >> 6] >> (c & 63)) & 1ull) << g;
        A.cls_bits[c] = bits;
    }
    const ClsArgs &args = A;
    if (side_launch_bin<bev_class_bin>(ctx, PCA_K_BEV_CLASS_BIN, args, s)) return -1;
    PCA_LAUNCH(ctx, PCA_K_BEV_CLASS_CELLS, bev_class_cells, dim3(args.s.T), dim3(CC_THREADS), s, args);
    PCA_CHECK(ctx, hipGetLastError());
    return 0;
}

}  // extern "C"
