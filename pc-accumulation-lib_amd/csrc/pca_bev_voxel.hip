// pca_bev_voxel.hip -- the BEV window voxelised into semantic occupancy labels: a counts-only pass with a height axis for gfx950.
//
// Semantic-occupancy ground truth (SemanticKITTI-SSC, SSCBench-KITTI-360) is the accumulated, labelled window voxelised with a
// majority vote per voxel.  The class planes (pca_bev_class.hip) count per (cell, set, group); this pass counts per (cell,
// height bin, label) and takes the argmax, on the same two-level scaffold (pca_bev_side.h: LDS atomics only, no global
// atomics); the view test, the cell and the owed re-transforms are pca_bev_view.h's.
//
//   level 1  bev_voxel_bin     side_bin with key = tile << 16 | cell_in_tile << 10 | k << 5 | label (a 1024^2 grid's 14 tile bits
//                              and these 16 stay below KEY_INVALID); the kept points' low 16 key bits are the record, one
//                              uint16_t.  The height bin k is floor(((Z - oz) + 0.0 - z_lo) / z_step) in f64 with the IEEE
//                              division; a point whose bin lies outside [0, nz) or whose label is 255 is dropped here.
//   level 2  bev_voxel_cells   side_tile_runs / side_find.  The tile's counters u32 [nz][n_labels][64 cells] are 256 KiB at 32 x 32:
//                              the workgroup walks the height axis in slabs of `zs` bins (64 zs n_labels 4 B of dynamic LDS,
//                              at most 56 KiB).  A tile's first 4 096 records stay in registers between the slabs, the rest
//                              is re-read from L2 (2 B each) once per slab: counts, barrier, argmax per voxel (the cell
//                              fastest: conflict-free LDS reads, eight lanes write one tile row).
// The order in which a tile's records arrive is not fixed (LDS cursors); counts and their argmax do not depend on it.
#include "pca_bev_voxel.h"

#define VB_REG_P 12               // points per thread of level 1 whose key stays in registers between its passes
#define VC_THREADS SIDE_CELLS_THREADS
#define VC_REG_R 16               // records per thread of level 2 that stay in registers between the slabs
#define VC_SLAB_COUNTERS 14336    // u32 counters of a slab at most: 56 KiB, which with side_tile_runs' tables stays below 64 KiB

// ---------------------------------------------------------------------------------------------
// level 1
// ---------------------------------------------------------------------------------------------
struct VoxBin {
    static constexpr int REG_P = VB_REG_P, SHIFT = 16;
    struct Payload {};
    const VoxArgs &v;
    const uint8_t *label_of;      // the table in LDS: the lookup hangs on the class word's load, a second trip to memory would show
    // key of stored point p: pca_bev_voxel.h's
    __device__ __forceinline__ uint32_t key(const SideArgs &, const ViewConst &vc, const PendHi &pend_hi, const SideWindow &, int64_t p, Payload &) const
    {
        return vox_point_key(v, vc, pend_hi, p, label_of);
    }
    __device__ __forceinline__ void dropped(const SideWindow &, int64_t) const {}
    __device__ __forceinline__ void store(int g, const SideWindow &w, uint32_t pos, uint32_t key, const Payload &, int64_t) const
    {
        v.recs[(int64_t)g * w.chunk + pos] = (uint16_t)(key & 0xffffu);
    }
};
__global__ __launch_bounds__(SIDE_BIN_THREADS) void bev_voxel_bin(const VoxArgs a)
{
    __shared__ uint8_t s_label[256];
    if (threadIdx.x < 256) s_label[threadIdx.x] = a.label_of[threadIdx.x];
    __syncthreads();
    side_bin(a.s, VoxBin{a, s_label});
}

// ---------------------------------------------------------------------------------------------
// level 2
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VC_THREADS) void bev_voxel_cells(const VoxArgs a)
{
    extern __shared__ uint32_t s_cnt[];                     // [zs][n_labels][64 cells]: the slab's counters
    __shared__ uint32_t s_pre[SIDE_PLACES + 1], s_off[SIDE_PLACES], s_wsum[VC_THREADS / 64];   // side_tile_runs
    const int tile = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int nl = a.n_labels, px = a.s.prm.px;
    int places;
    const uint32_t total = side_tile_runs(a.s, tile, s_pre, s_off, s_wsum, places);
    const int row0 = (tile / a.s.tx) * TS, col0 = (tile % a.s.tx) * TS;
    const size_t plane = (size_t)px * px;
    // the tile's first VC_REG_R x 256 records (a headline tile: all of them) are found and read once, for every slab
    uint32_t regs[VC_REG_R];
#pragma unroll
    for (int i = 0; i < VC_REG_R; ++i) {
        const uint32_t r = (uint32_t)(i * VC_THREADS + tid);
        regs[i] = ~0u;                                      // (no record: a record is below 1 << 16)
        if (r < total) {
            const int lo = side_find(s_pre, places, r);
            regs[i] = a.recs[(size_t)s_off[lo] + (r - s_pre[lo])];
        }
    }
    for (int z0 = 0; z0 < a.nz; z0 += a.zs) {
        const int zn = a.nz - z0 < a.zs ? a.nz - z0 : a.zs;
        for (int i = tid; i < zn * nl * TCELLS; i += VC_THREADS) s_cnt[i] = 0;
        __syncthreads();
        // one LDS atomic for a record of this slab; what the registers do not hold: place by binary search over the prefix table
#pragma unroll
        for (int i = 0; i < VC_REG_R; ++i) {
            const uint32_t rec = regs[i];
            const uint32_t k = ((rec >> 5) & 31u) - (uint32_t)z0;
            if (rec < 0x10000u && k < (uint32_t)zn) atomicAdd(&s_cnt[(k * nl + (rec & 31u)) * TCELLS + (rec >> 10)], 1u);
        }
        for (uint32_t r = VC_REG_R * VC_THREADS + tid; r < total; r += VC_THREADS) {
            const int lo = side_find(s_pre, places, r);
            const uint32_t rec = a.recs[(size_t)s_off[lo] + (r - s_pre[lo])];
            const uint32_t k = ((rec >> 5) & 31u) - (uint32_t)z0;   // (wraps to a large number below the slab)
            if (k < (uint32_t)zn) atomicAdd(&s_cnt[(k * nl + (rec & 31u)) * TCELLS + (rec >> 10)], 1u);
        }
        __syncthreads();
        // argmax per voxel: item = (bin, cell), the cell fastest -- eight lanes write one row of the tile
        for (int i = tid; i < zn * TCELLS; i += VC_THREADS) {
            const int cell = i & 63, k = i >> 6;
            const int row = row0 + (cell >> 3), col = col0 + (cell & 7);
            if (row >= px || col >= px) continue;
            const uint32_t *c = s_cnt + (size_t)k * nl * TCELLS + cell;
            uint32_t n = 0, best = 0, label = 255u;
            for (int l = 0; l < nl; ++l) {
                const uint32_t n_l = c[l * TCELLS];
                n += n_l;
                if (n_l > best) { best = n_l; label = (uint32_t)l; }   // strict: of equal counts the smallest label stays
            }
            const size_t at = (size_t)(z0 + k) * plane + (size_t)row * px + col;
            if (a.labels) a.labels[at] = (uint8_t)label;
            if (a.counts) a.counts[at] = n;
            if (a.top) a.top[at] = best;
        }
        __syncthreads();                                    // (the next slab clears what this one read)
    }
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
// the workspace: the uint16_t records, then the table (side_layout)
static SideLayout vox_layout(int64_t max_points, int px) { return side_layout(max_points, px, 2, 0, "PCA_BEV_VOXEL_G"); }
static const WindowPass VOX_PASS = {"bev voxel labels", true, false};

int64_t bev_voxel_workspace(int64_t max_points, int px) { return vox_layout(max_points, px).total; }

int bev_voxel_prepare(pca_ctx *ctx, const WindowPass &pass, bool own_ok, const pca_store *store, const int64_t *frame_off,
                      int slot_begin, int slot_end, int64_t max_points, const pca_bev_params *prm, double z_lo, double z_step,
                      int nz, const uint8_t *label_of, int n_labels, int dyn_mode, const double *pending_Ts,
                      const int *pending_slot_ends, int n_pending, void *workspace, int64_t workspace_bytes, VoxArgs &A)
{
    const std::string what(pass.what);
    char *w;
    if (window_check(ctx, pass, label_of && workspace && own_ok, store, frame_off, slot_begin, slot_begin, slot_end, max_points,
                     prm, pending_Ts, pending_slot_ends, n_pending, A.s))
        return -1;
    if (voxel_grid_check(ctx, pass.what, z_lo, z_step, nz)) return -1;
    if (n_labels < 1 || n_labels > PCA_BEV_VOXEL_MAX_LABELS) { ctx->err = what + ": n_labels must be in 1..32"; return -1; }
    for (int c = 0; c < 256; ++c)
        if (label_of[c] != 255 && label_of[c] >= n_labels) {
            ctx->err = what + ": label_of[" + std::to_string(c) + "] must be below n_labels, or 255";
            return -1;
        }
    if (side_tiles(ctx, pass.what, slot_begin, workspace, workspace_bytes, vox_layout(max_points, prm->px), A.s, w)) return -1;
    A.z_lo = z_lo; A.z_step = z_step;
    A.nz = nz; A.n_labels = n_labels; A.dyn_mode = dyn_mode;
    // the slabs of level 2: as few as the counters allow, then of equal height
    const int zs_max = VC_SLAB_COUNTERS / (TCELLS * n_labels);
    const int n_slabs = (nz + zs_max - 1) / zs_max;
    A.zs = (nz + n_slabs - 1) / n_slabs;
    A.recs = reinterpret_cast<uint16_t *>(w);
    A.labels = nullptr; A.counts = nullptr; A.top = nullptr;
    for (int c = 0; c < 256; ++c) A.label_of[c] = label_of[c];
    return 0;
}

int bev_voxel_enqueue(pca_ctx *ctx, const VoxArgs &args, hipStream_t s)
{
    if (side_launch_bin<bev_voxel_bin>(ctx, PCA_K_BEV_VOXEL_BIN, args, s)) return -1;
    PCA_LAUNCH_SHM(ctx, PCA_K_BEV_VOXEL_CELLS, bev_voxel_cells, dim3(args.s.T), dim3(VC_THREADS),
                   (size_t)args.zs * args.n_labels * TCELLS * 4, s, args);
    return 0;
}

extern "C" {

int64_t pca_bev_voxel_workspace_bytes(int64_t max_points, int px) { return bev_voxel_workspace(max_points, px); }

int pca_bev_voxel_labels(pca_ctx *ctx, const pca_store *store, const int64_t *frame_off, int slot_begin, int slot_end,
                         int64_t max_points, const pca_bev_params *prm, double z_lo, double z_step, int nz,
                         const uint8_t label_of[256], int n_labels, int include_dyn, const double *pending_Ts,
                         const int *pending_slot_ends, int n_pending, void *workspace, int64_t workspace_bytes,
                         uint8_t *labels, uint32_t *counts, uint32_t *top, void *stream)
{
    if (!ctx) return -1;
    if (max_points < 1) max_points = 1;
    // every check comes before the first launch (a noted K1 included)
    VoxArgs A;
    if (bev_voxel_prepare(ctx, VOX_PASS, labels || counts || top, store, frame_off, slot_begin, slot_end, max_points, prm, z_lo,
                          z_step, nz, label_of, n_labels, include_dyn != 0 ? 1 : 0, pending_Ts, pending_slot_ends, n_pending,
                          workspace, workspace_bytes, A))
        return -1;
    A.labels = labels; A.counts = counts; A.top = top;
    if (bev_voxel_enqueue(ctx, A, (hipStream_t)stream)) return -1;
    PCA_CHECK(ctx, hipGetLastError());
    return 0;
}

}  // extern "C"
