// pca_bev_voxel.h -- what the passes over the voxel grid share with pca_bev_voxel.hip (the occupancy labels; the instances of
// pca_bev_inst.hip): the argument block, the ONE copy of a stored point's voxel key and the host entry that checks a call
// and enqueues the two levels of the voxel pass.
#pragma once
#include "pca_bev_side.h"

struct alignas(16) VoxArgs {
    SideArgs s;                   // (slot_split = slot_begin: the voxels know no sets)
    double z_lo, z_step;
    int nz, n_labels;
    int dyn_mode;                 // 0: points with dyn == 1 take no part; 1: every point; 2: only points with dyn == 1
    int zs;                       // height bins per slab of level 2
    uint16_t *recs;               // [max_points + G]: cell_in_tile << 10 | k << 5 | label, tile-ordered per segment
    uint8_t *labels;              // [nz][px][px] or NULL
    uint32_t *counts, *top;       // [nz][px][px] or NULL
    uint8_t label_of[256];        // class -> label, 255: the class takes no part
};

// Key of stored point p: tile << 16 | cell_in_tile << 10 | k << 5 | label, or KEY_INVALID (not kept).  The view's key (tile <<
// 7 | cell_in_tile << 1 | set, set = 0) >> 1, then the height bin and the label; label_of: the table wherever the caller
// keeps it (level 1: in LDS).
__device__ __forceinline__ uint32_t vox_point_key(const VoxArgs &v, const ViewConst &vc, const PendHi &pend_hi, int64_t p,
                                                  const uint8_t *label_of)
{
    const SideArgs &a = v.s;
    double X = pca_ldg(a.st.x + p), Y = pca_ldg(a.st.y + p), Z = pca_ldg(a.st.z + p);
    const uint8_t D = pca_ldg(a.st.dyn + p);
    apply_owed(a.owed, pend_hi, p, X, Y, Z);
    const bool live = v.dyn_mode == 2 ? D == 1 : (v.dyn_mode != 0 || D != 1);
    const uint32_t vk = view_key_lean<false>(vc, X, Y, Z, live, 0u);
    if (vk == KEY_INVALID) return KEY_INVALID;
    const uint32_t label = label_of[pca_ldg(a.st.rgbs + p) >> 24];    // (the class byte: read for the kept points only)
    const double z = (Z - vc.oz) + 0.0;
    const double kf = floor((z - v.z_lo) / v.z_step);       // the IEEE division: no reciprocal, nothing fused
    if (label == 255u || !(kf >= 0.0 && kf < (double)v.nz)) return KEY_INVALID;   // in z nothing is clamped
    return ((vk >> 1) << 10) | ((uint32_t)(int)kf << 5) | label;
}
// the key's place in the [nz][px][px] output (image rows)
__device__ __forceinline__ uint32_t vox_key_place(uint32_t key, int tx, int px)
{
    const uint32_t tile = key >> 16, cell = (key >> 10) & 63u, k = (key >> 5) & 31u;
    const uint32_t row = (tile / (uint32_t)tx) * TS + (cell >> 3), col = (tile % (uint32_t)tx) * TS + (cell & 7u);
    return (k * (uint32_t)px + row) * (uint32_t)px + col;
}

// ---- host side (pca_bev_voxel.hip) ----
int64_t bev_voxel_workspace(int64_t max_points, int px);
// Every check of a pass over the voxel grid (window, grid, label table, workspace of bev_voxel_workspace bytes) under the
// pass's own message prefix, before anything is launched; fills A but for its outputs.  own_ok: the pass's own pointers.
int bev_voxel_prepare(pca_ctx *ctx, const WindowPass &pass, bool own_ok, const pca_store *store, const int64_t *frame_off,
                      int slot_begin, int slot_end, int64_t max_points, const pca_bev_params *prm, double z_lo, double z_step,
                      int nz, const uint8_t *label_of, int n_labels, int dyn_mode, const double *pending_Ts,
                      const int *pending_slot_ends, int n_pending, void *workspace, int64_t workspace_bytes, VoxArgs &A);
// a noted K1 first, then level 1 and level 2 into A's outputs
int bev_voxel_enqueue(pca_ctx *ctx, const VoxArgs &A, hipStream_t s);
