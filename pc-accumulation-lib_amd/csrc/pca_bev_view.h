// pca_bev_view.h -- what every pass that bins the window into 8x8-cell BEV tiles shares (the main rasteriser pca_bev.hip, the
// class planes pca_bev_class.hip, the elevation partition pca_bev_elev.hip): the tile side, the view test and cell function,
// the chain of owed re-transforms (device and host side) and the XCD-major order of the per-(tile, workgroup) tables.
// The ONE copy of each: tests/test_gpu_bev_edges.py and tests/test_gpu_bev_side_edges.py pin its edge behaviour to the reference.
#pragma once
#include "pca_common.h"

#define KEY_INVALID 0xffffffffu
#define TS 8                      // tile side [cells]
#define TCELLS (TS * TS)

// The view test and cell key of one point, written for instruction count (level 1 is bound by vector issue, not by memory:
// ~270 instructions per point before, a third of them v_readlane of spilled scalars).  Same values as the reference's full
// 3x3 chain: R is a rotation about z (checked by the host, bev_check_rotation), so R[2] z, R[5] z, R[6] x and R[7] y are exact
// zeros and R[8] z is z -- for FINITE z; a point whose z is not finite is dropped here, as the reference drops it (0 * inf =
// NaN poisons its x and y).
struct ViewConst { double ox, oy, oz, r0, r1, r3, r4, dx, dy, vlo, vhi, v, rv, pxd, half_px, hf; int px, tx; bool use_h; uint32_t br0, brows; };
__device__ __forceinline__ ViewConst view_const(const pca_bev_params &q, int tx, int band_r0, int band_rows)
{
    ViewConst c;
    c.ox = q.origin[0]; c.oy = q.origin[1]; c.oz = q.origin[2];
    c.r0 = q.R[0]; c.r1 = q.R[1]; c.r3 = q.R[3]; c.r4 = q.R[4];
    c.dx = q.dx; c.dy = q.dy;
    c.v = q.view; c.rv = 1.0 / q.view; c.vlo = -0.5 * q.view; c.vhi = 0.5 * q.view; c.pxd = (double)q.px; c.half_px = 0.5 * c.pxd;
    // (handing 1 / view, (double)px and px / 2 over from the host instead was measured: 57.7-57.8 us against 56.8-57.2)
    c.hf = q.height_filter; c.use_h = !(q.height_filter != q.height_filter);
    c.px = q.px; c.tx = tx;
    c.br0 = (uint32_t)band_r0; c.brows = (uint32_t)band_rows;   // (read by the BAND variant only)
    return c;
}
// key = tile << 7 | cell_in_tile << 1 | set of a point with stored coordinates X, Y, Z (after the owed transforms); KEY_INVALID
// = not in the view, or not `live`.
// BAND (banded rasters, px > 1024): i, j, the clamp and the row are those of the FULL grid; a point whose tile row lies outside
// the band [br0, br0 + brows) gets KEY_INVALID, the others the key of their tile numbered within the band.
template <bool BAND = false>
__device__ __forceinline__ uint32_t view_key_lean(const ViewConst &c, double X, double Y, double Z, bool live, uint32_t set)
{
    const double x = X - c.ox, y = Y - c.oy;
    const double ax = fma(c.r1, y, c.r0 * x) + c.dx;
    const double ay = fma(c.r4, y, c.r3 * x) + c.dy;
    bool keep = live && (ax > c.vlo) && (ax < c.vhi) && (ay > c.vlo) && (ay < c.vhi) && (fabs(Z) < __builtin_huge_val());
    if (c.use_h) keep = keep && (Z - c.oz < c.hf);
    uint32_t key = KEY_INVALID;
    if (keep) {
        // floor(a / view * px + px / 2), the reference's expression.  The IEEE division (~22 instructions) is replaced by
        // the quotient estimate  q = a rv,  q += fma(-q, view, a) rv  (within one ulp of the rounded quotient): the floor
        // can only differ if the sum lands within a few ulps of an integer, and a sum within 1e-9 of one is recomputed
        // with the real division (about two points in a billion).  The margin holds up to the largest grid, px = 4096: |q| < 1/2,
        // so ulp(q) px <= 2^-53 * 4096 ~ 4.5e-13, far below 1e-9.
        const double qx0 = ax * c.rv, qy0 = ay * c.rv;
        const double qx = fma(fma(-qx0, c.v, ax), c.rv, qx0), qy = fma(fma(-qy0, c.v, ay), c.rv, qy0);
        double tx = qx * c.pxd + c.half_px, ty = qy * c.pxd + c.half_px;
        double fx = floor(tx), fy = floor(ty);
        if ((tx - fx < 1e-9) | (fx + 1.0 - tx < 1e-9) | (ty - fy < 1e-9) | (fy + 1.0 - ty < 1e-9)) {
            fx = floor(ax / c.v * c.pxd + c.half_px);
            fy = floor(ay / c.v * c.pxd + c.half_px);
        }
        int i = (int)fx;
        int j = (int)fy;
        i = i > c.px - 1 ? c.px - 1 : (i < 0 ? 0 : i);
        j = j > c.px - 1 ? c.px - 1 : (j < 0 ? 0 : j);
        const uint32_t row = (uint32_t)(c.px - 1 - j), col = (uint32_t)i;
        const uint32_t trow = BAND ? row / TS - c.br0 : row / TS;   // (BAND: wraps to a large number above the band)
        const uint32_t tile = trow * (uint32_t)c.tx + (col / TS);
        if (!BAND || trow < c.brows) key = (tile << 7) | ((((row % TS) * TS + (col % TS)) * 2u) + set);
    }
    return key;
}

// The owed re-transforms of a window, oldest first: transform k is owed by slots [slot_begin, pend_slot_end[k]) (ascending).
// write_back: the pass also stores the moved points (the main raster alone; else they are applied to what the pass reads and
// stay owed).  It sits here, between n_pend and the slot ends, so that every field of the main raster's argument block keeps
// the offset its kernels were tuned with (level 1's scalar register spills follow the offsets).
struct BevOwed { int n_pend; int write_back; int pend_slot_end[PCA_BEV_MAX_CHAIN]; Mat34 pend_T[PCA_BEV_MAX_CHAIN]; };
struct PendHi { int64_t v[PCA_BEV_MAX_CHAIN]; };           // first point index that does NOT owe transform k
// (frame_off lives on the device; lo: the window's first point -- a transform no slot of the window owes ends there)
__device__ __forceinline__ PendHi owed_bounds(const BevOwed &o, const int64_t *frame_off, int slot_begin, int64_t lo)
{
    PendHi pend_hi;
#pragma unroll
    for (int k = 0; k < PCA_BEV_MAX_CHAIN; ++k)
        pend_hi.v[k] = (k < o.n_pend && o.pend_slot_end[k] > slot_begin) ? frame_off[o.pend_slot_end[k]] : lo;
    return pend_hi;
}
// the owed re-transforms of point p, oldest first, each a separate fma chain (the roundings of one K2 pass per
// transform); returns whether the point owed any
__device__ __forceinline__ bool apply_owed(const BevOwed &o, const PendHi &pend_hi, int64_t p, double &X, double &Y, double &Z)
{
    bool moved = false;
#pragma unroll 1                                            // (not unrolled: the coefficients are fetched when their turn
    for (int k = 0; k < o.n_pend; ++k) {                    //  comes -- unrolled, all 48 are preloaded into scalar registers
        const int64_t hi = k == 0 ? pend_hi.v[0] : k == 1 ? pend_hi.v[1] : k == 2 ? pend_hi.v[2] : pend_hi.v[3];   // and spill)
        if (p < hi) {
            const Mat34 &T = o.pend_T[k];
            const double nx = row4(T.m + 0, X, Y, Z), ny = row4(T.m + 4, X, Y, Z), nz = row4(T.m + 8, X, Y, Z);
            X = nx; Y = ny; Z = nz;
            moved = true;
        }
    }
    return moved;
}

// The per-(tile, workgroup) tables of level 1 are [tile][Gr] with workgroup g at position (g mod 8) Gp + g / 8:
// workgroups are dealt to the eight XCDs round-robin, so the entries that share a cache line are written by workgroups of
// ONE XCD -- the 32 of a round fill a whole 128-byte line in that XCD's L2, which then leaves it as one full-line write.
// In plain [tile][g] order a line held the 4-byte stores of eight different L2s: 1 M partial-line writes per call, 100 MB
// of write traffic for 75 MB of payload.  Level 2 reads a tile's row as one range either way.  Gp = 0: plain order.
__device__ __forceinline__ int bev_table_pos(int Gp, int g) { return Gp ? (g & 7) * Gp + (g >> 3) : g; }
__device__ __forceinline__ int bev_table_group(int Gp, int p)
{
    if (!Gp) return p;
    const int x = p / Gp;
    return (p - x * Gp) * 8 + x;                            // may be >= G: an unused place of the row
}

// ---- host side: the argument checks the entry points share.  `what` is the message prefix ("bev", "bev class planes",
// "bev elev partition", ...); on failure ctx->err is set and -1 returned. ----
// the elevation is min(z - origin_z) and the cell function drops R's third row and column: the rotation has to leave z alone
// (rotation_matrix_3d of the reference)
static inline int bev_check_rotation(pca_ctx *ctx, const char *what, const pca_bev_params *prm)
{
    if (prm->R[6] == 0.0 && prm->R[7] == 0.0 && prm->R[8] == 1.0 && prm->R[2] == 0.0 && prm->R[5] == 0.0) return 0;
    ctx->err = std::string(what) + ": R must be a rotation about the z axis (R[2] = R[5] = R[6] = R[7] = 0, R[8] = 1)";
    return -1;
}
// checks the caller's chain (n_pending 4x4 row-major transforms and their slot ends) against the window and copies it
static inline int bev_fill_owed(pca_ctx *ctx, const char *what, const double *pending_Ts, const int *pending_slot_ends, int n_pending,
                                int slot_begin, int slot_end, BevOwed &o)
{
    const std::string w(what);
    if (n_pending < 0 || n_pending > PCA_BEV_MAX_CHAIN || (n_pending > 0 && (!pending_Ts || !pending_slot_ends))) {
        ctx->err = w + ": bad chain of owed transforms";
        return -1;
    }
    o.n_pend = n_pending;
    o.write_back = 0;                                       // (the main raster sets it)
    for (int k = 0; k < PCA_BEV_MAX_CHAIN; ++k) {
        o.pend_slot_end[k] = slot_begin;
        for (int i = 0; i < 12; ++i) o.pend_T[k].m[i] = 0.0;
        if (k >= n_pending) continue;
        if (pending_slot_ends[k] > slot_end) { ctx->err = w + ": a pending slot end lies beyond the window"; return -1; }
        if (k > 0 && pending_slot_ends[k] < pending_slot_ends[k - 1]) { ctx->err = w + ": pending slot ends must ascend"; return -1; }
        o.pend_slot_end[k] = pending_slot_ends[k];
        for (int i = 0; i < 12; ++i) o.pend_T[k].m[i] = pending_Ts[16 * k + i];
    }
    return 0;
}

// ---- host side: a read-only pass over a window of the store (the class planes, the elevation partition, the occupancy labels,
// the rays through the voxel grid, the camera render of pca_render.hip; the next pass of the family starts here).  The main
// raster has its own checks. ----
#define SIDE_PX_MAX 1024          // the largest grid of these passes (no banding)
// what: the message prefix; rgbs: the pass reads the class byte; split: its window has a slot_split
struct WindowPass { const char *what; bool rgbs, split; };
// The checks every entry point shares, before anything is launched, whatever the pass renders into (a BEV grid or a camera
// image): the pointers (own_ok: those of the pass's own arguments, its parameter block included), the store's arrays, the slot
// order, then the pass's own `target` check (a callable returning 0 or -1 with ctx->err set: the grid of the BEV passes),
// the owed chain -- and the fields every argument block has (Args: SideArgs, RayArgs or RenderArgs; a pass without a split
// hands slot_begin in its place).
template <typename Args, typename Target>
static inline int window_check_any(pca_ctx *ctx, const WindowPass &pass, bool own_ok, const pca_store *store, const int64_t *frame_off,
                                   int slot_begin, int slot_split, int slot_end, int64_t max_points, Target target,
                                   const double *pending_Ts, const int *pending_slot_ends, int n_pending, Args &A)
{
    const std::string w(pass.what);
    if (!store || !frame_off || !own_ok) { ctx->err = w + ": bad arguments"; return -1; }
    if (!store->x || !store->y || !store->z || (pass.rgbs && !store->rgbs) || !store->dyn) {
        ctx->err = w + ": the store's x, y, z" + (pass.rgbs ? ", rgbs" : "") + " and dyn arrays are needed";
        return -1;
    }
    if (!(slot_begin <= slot_split && slot_split <= slot_end)) {
        ctx->err = w + (pass.split ? ": need slot_begin <= slot_split <= slot_end" : ": need slot_begin <= slot_end");
        return -1;
    }
    if (target()) return -1;
    if (bev_fill_owed(ctx, pass.what, pending_Ts, pending_slot_ends, n_pending, slot_begin, slot_end, A.owed)) return -1;
    A.st = *store;
    A.frame_off = frame_off;
    A.slot_begin = slot_begin; A.slot_end = slot_end;
    A.max_points = max_points;
    A.status = ctx->ticket + 1;
    return 0;
}
// ... of a pass over a BEV grid: px and the rotation between the slot order and the owed chain, prm into the block.
template <typename Args>
static inline int window_check(pca_ctx *ctx, const WindowPass &pass, bool own_ok, const pca_store *store, const int64_t *frame_off,
                               int slot_begin, int slot_split, int slot_end, int64_t max_points, const pca_bev_params *prm,
                               const double *pending_Ts, const int *pending_slot_ends, int n_pending, Args &A)
{
    auto grid = [&]() -> int {
        if (prm->px < 1 || prm->px > SIDE_PX_MAX) { ctx->err = std::string(pass.what) + ": px must be in 1..1024"; return -1; }
        return bev_check_rotation(ctx, pass.what, prm);
    };
    if (window_check_any(ctx, pass, prm && own_ok, store, frame_off, slot_begin, slot_split, slot_end, max_points, grid,
                         pending_Ts, pending_slot_ends, n_pending, A))
        return -1;
    A.prm = *prm;
    return 0;
}
// the voxel grid of the occupancy labels and of the rays: nz height bins of z_step from z_lo
static inline int voxel_grid_check(pca_ctx *ctx, const char *what, double z_lo, double z_step, int nz)
{
    const std::string w(what);
    if (nz < 1 || nz > PCA_BEV_VOXEL_MAX_Z) { ctx->err = w + ": nz must be in 1..32"; return -1; }
    if (!(fabs(z_lo) < __builtin_huge_val())) { ctx->err = w + ": z_lo must be finite"; return -1; }
    if (!(z_step > 0.0 && z_step < __builtin_huge_val())) { ctx->err = w + ": z_step must be finite and > 0"; return -1; }
    return 0;
}
