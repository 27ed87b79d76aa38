// pca_bev_class.hip -- BEV planes of any semantic class group: a counts-only pass over the window for gfx950.
//
// The main rasteriser (pca_bev.hip) turns two class sets into planes, `road` and the vehicle set, next to exact medians,
// minimum z and intensity sums.  A class plane needs none of those: per (cell, set) the number of static points and, per
// group, the number of them whose class is in the group.  This file counts ALL groups in one pass that reads 29 bytes per
// stored point (x, y, z, dyn and -- for the points inside the view -- the class byte inside rgbs), with the rasteriser's
// structure: two levels, LDS atomics only, no global atomics (a one-dword-per-lane scatter of global atomics runs at the
// memory side on this part, an order of magnitude below the streaming rate).
//
//   level 1  bev_class_bin     1024 threads; workgroup g takes chunk g of the window: owed re-transforms, view test and cell
//                              exactly as view_key of pca_bev.hip spells them out -> key = tile << 15 | cell_in_tile << 9 |
//                              set << 8 | class; LDS histogram over the 8x8-cell tiles (4 B per tile: 64 KiB at 1024^2);
//                              exclusive scan IN PLACE (the histogram becomes the cursors); the kept points' low 15 key bits
//                              -- one uint16_t record -- sorted by tile into the workgroup's own segment; {count, offset}
//                              per (tile, workgroup) into the table.  The first CB_REG_P x 1024 points of a chunk keep their
//                              key in registers between the passes (a 200-frame KITTI window: all of it); what a chunk holds
//                              beyond that is recomputed from L2.
//   level 2  bev_class_cells   256 threads, one workgroup per tile: prefix table over the workgroups' runs in LDS, binary
//                              search per record, counts into LDS u32 [64 cells][2 sets][n_groups + 1] through the table
//                              class -> bit set of its groups (groups may overlap; the last slot counts every static point),
//                              closed form per (cell, set, group), whole tile rows written.
// The order in which a tile's records arrive is not fixed (LDS cursors); counts do not depend on it.
#include "pca_common.h"

#define CB_THREADS 1024           // workgroup size of level 1
#define CB_REG_P 12               // points per thread of level 1 whose key stays in registers between its passes
#define CB_MAX_G 512              // workgroups of level 1 at most (two rounds of one per CU)
#define CB_CHUNK 8192             // points per workgroup of level 1 the launch is sized for
#define CC_THREADS 256            // workgroup size of level 2
#define CC_TS 8                   // tile side [cells]
#define CC_MAX_S (PCA_BEV_MAX_CLASS_GROUPS + 1)   // counters per (cell, set)
#define CLS_PX_MAX 1024
#define CLS_KEY_INVALID 0xffffffffu

struct alignas(16) ClsArgs {
    pca_store st;
    const int64_t *frame_off;
    int slot_begin, slot_split, slot_end;
    int64_t max_points;
    pca_bev_params prm;
    int n_pend;                   // owed re-transforms, oldest first: transform k is owed by slots [slot_begin, pend_slot_end[k])
    int pend_slot_end[PCA_BEV_MAX_CHAIN];
    Mat34 pend_T[PCA_BEV_MAX_CHAIN];
    int tx, T;                    // tiles per row, tiles
    int G;                        // workgroups of level 1; 0: the window holds no slot, level 2 alone writes the prior
    int Gr, Gp;                   // the table's row length (>= G) and workgroups per XCD column block (cls_table_pos)
    int n_groups;
    uint16_t *recs;               // [max_points + G]: cell_in_tile << 9 | set << 8 | class, tile-ordered per segment
    uint2 *table;                 // [T][Gr] {kept records, offset in the segment} per (tile, workgroup)
    double *prob;                 // [3][n_groups][px][px] or NULL
    uint16_t *prob_f16;           // the same as f16 bits or NULL
    uint32_t *counts;             // [3][n_groups + 1][px][px] or NULL
    uint32_t *status;             // context status word (PCA_STATUS_* bits)
    uint32_t cls_bits[256];       // class -> bit g: the class is in group g; bit n_groups: always (every static point)
};

struct ClsWindow { int64_t lo, hi, sp, chunk; };
// the window as both kernels see it (frame_off lives on the device); above max_points it is cut, as the main raster cuts it
__device__ __forceinline__ ClsWindow cls_window(const ClsArgs &a)
{
    ClsWindow w;
    w.lo = a.frame_off[a.slot_begin];
    const int64_t hi0 = a.frame_off[a.slot_end];
    w.sp = a.frame_off[a.slot_split];
    w.hi = (hi0 - w.lo > a.max_points) ? w.lo + a.max_points : hi0;
    const int G = a.G > 0 ? a.G : 1;
    w.chunk = (w.hi - w.lo + G - 1) / G;
    return w;
}
// The table is [tile][Gr] with workgroup g at position (g mod 8) Gp + g / 8, as the main raster's counter tables are:
// workgroups are dealt to the eight XCDs round-robin, so the entries that share a cache line come from ONE XCD's L2 and leave
// it as full lines.  Gp = 0: plain order.
__device__ __forceinline__ int cls_table_pos(const ClsArgs &a, int g) { return a.Gp ? (g & 7) * a.Gp + (g >> 3) : g; }
__device__ __forceinline__ int cls_table_group(const ClsArgs &a, int p)
{
    if (!a.Gp) return p;
    const int x = p / a.Gp;
    return (p - x * a.Gp) * 8 + x;                          // may be >= G: an unused place of the row
}

// The view test and the cell of one point, the main raster's (view_key of pca_bev.hip; R is a rotation about z, checked by
// the host, so R[2] z, R[5] z, R[6] x and R[7] y are exact zeros and R[8] z is z for finite z; a point whose z is not finite
// is dropped, as the reference drops it: 0 * inf = NaN poisons its x and y).
struct ClsView { double ox, oy, oz, r0, r1, r3, r4, dx, dy, vlo, vhi, v, rv, pxd, half_px, hf; int px, tx; bool use_h; };
__device__ __forceinline__ ClsView cls_view(const ClsArgs &a)
{
    const pca_bev_params &q = a.prm;
    ClsView c;
    c.ox = q.origin[0]; c.oy = q.origin[1]; c.oz = q.origin[2];
    c.r0 = q.R[0]; c.r1 = q.R[1]; c.r3 = q.R[3]; c.r4 = q.R[4];
    c.dx = q.dx; c.dy = q.dy;
    c.v = q.view; c.rv = 1.0 / q.view; c.vlo = -0.5 * q.view; c.vhi = 0.5 * q.view; c.pxd = (double)q.px; c.half_px = 0.5 * c.pxd;
    c.hf = q.height_filter; c.use_h = !(q.height_filter != q.height_filter);
    c.px = q.px; c.tx = a.tx;
    return c;
}
struct ClsPendHi { int64_t v[PCA_BEV_MAX_CHAIN]; };         // first point index that does NOT owe transform k
// the owed re-transforms of point p, oldest first, each a separate fma chain (the roundings of one K2 pass per transform)
__device__ __forceinline__ void cls_apply_owed(const ClsArgs &a, const ClsPendHi &pend_hi, int64_t p, double &X, double &Y, double &Z)
{
#pragma unroll 1                                            // (the coefficients are fetched when their turn comes)
    for (int k = 0; k < a.n_pend; ++k) {
        const int64_t hi = k == 0 ? pend_hi.v[0] : k == 1 ? pend_hi.v[1] : k == 2 ? pend_hi.v[2] : pend_hi.v[3];
        if (p < hi) {
            const Mat34 &T = a.pend_T[k];
            const double nx = row4(T.m + 0, X, Y, Z), ny = row4(T.m + 4, X, Y, Z), nz = row4(T.m + 8, X, Y, Z);
            X = nx; Y = ny; Z = nz;
        }
    }
}
// key of stored point p: tile << 15 | cell_in_tile << 9 | set << 8 | class, CLS_KEY_INVALID = not counted
__device__ __forceinline__ uint32_t cls_key(const ClsArgs &a, const ClsView &c, const ClsPendHi &pend_hi, int64_t sp, int64_t p)
{
    double X = pca_ldg(a.st.x + p), Y = pca_ldg(a.st.y + p), Z = pca_ldg(a.st.z + p);
    const uint8_t D = pca_ldg(a.st.dyn + p);
    cls_apply_owed(a, pend_hi, p, X, Y, Z);
    const double x = X - c.ox, y = Y - c.oy;
    const double ax = fma(c.r1, y, c.r0 * x) + c.dx;
    const double ay = fma(c.r4, y, c.r3 * x) + c.dy;
    bool keep = (D != 1) && (ax > c.vlo) && (ax < c.vhi) && (ay > c.vlo) && (ay < c.vhi) && (fabs(Z) < __builtin_huge_val());
    if (c.use_h) keep = keep && (Z - c.oz < c.hf);
    if (!keep) return CLS_KEY_INVALID;
    // floor(a / view * px + px / 2), the reference's expression, with the main raster's shortcut: the quotient estimate
    // q = a rv, q += fma(-q, view, a) rv lies within one ulp of the rounded quotient, so the floor can only differ if the sum
    // lands within a few ulps of an integer; a sum within 1e-9 of one is recomputed with the real division.
    const double qx0 = ax * c.rv, qy0 = ay * c.rv;
    const double qx = fma(fma(-qx0, c.v, ax), c.rv, qx0), qy = fma(fma(-qy0, c.v, ay), c.rv, qy0);
    const double tx = qx * c.pxd + c.half_px, ty = qy * c.pxd + c.half_px;
    double fx = floor(tx), fy = floor(ty);
    if ((tx - fx < 1e-9) | (fx + 1.0 - tx < 1e-9) | (ty - fy < 1e-9) | (fy + 1.0 - ty < 1e-9)) {
        fx = floor(ax / c.v * c.pxd + c.half_px);
        fy = floor(ay / c.v * c.pxd + c.half_px);
    }
    int i = (int)fx, j = (int)fy;
    i = i > c.px - 1 ? c.px - 1 : (i < 0 ? 0 : i);
    j = j > c.px - 1 ? c.px - 1 : (j < 0 ? 0 : j);
    const uint32_t row = (uint32_t)(c.px - 1 - j), col = (uint32_t)i;
    const uint32_t tile = (row / CC_TS) * (uint32_t)c.tx + col / CC_TS;
    const uint32_t cell = (row % CC_TS) * CC_TS + col % CC_TS;
    const uint32_t cls = pca_ldg(a.st.rgbs + p) >> 24;      // (read for the kept points only)
    return (tile << 15) | (cell << 9) | ((p >= sp ? 1u : 0u) << 8) | cls;
}

// ---------------------------------------------------------------------------------------------
// level 1
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CB_THREADS) void bev_class_bin(const ClsArgs a)
{
    extern __shared__ uint32_t s_h[];                       // [T]: histogram over the tiles, after the scan the cursors
    __shared__ uint32_t s_wsum[CB_THREADS / 64];
    const int g = (int)blockIdx.x, tid = (int)threadIdx.x;
    const ClsWindow w = cls_window(a);
    int64_t c_lo = w.lo + (int64_t)g * w.chunk;
    int64_t c_hi = c_lo + w.chunk < w.hi ? c_lo + w.chunk : w.hi;
    if (c_lo > w.hi) c_lo = c_hi = w.hi;
    if (g == 0 && tid == 0 && a.frame_off[a.slot_end] - w.lo > a.max_points) pca_raise(a.status, PCA_STATUS_STORE_OVERFLOW);
    for (int t = tid; t < a.T; t += CB_THREADS) s_h[t] = 0;
    __syncthreads();
    ClsPendHi pend_hi;
#pragma unroll
    for (int k = 0; k < PCA_BEV_MAX_CHAIN; ++k)
        pend_hi.v[k] = (k < a.n_pend && a.pend_slot_end[k] > a.slot_begin) ? a.frame_off[a.pend_slot_end[k]] : w.lo;
    const ClsView vc = cls_view(a);
    // pass A: keys and the histogram
    uint32_t keys[CB_REG_P];
#pragma unroll
    for (int k = 0; k < CB_REG_P; ++k) {
        const int64_t p = c_lo + (int64_t)k * CB_THREADS + tid;
        keys[k] = p < c_hi ? cls_key(a, vc, pend_hi, w.sp, p) : CLS_KEY_INVALID;
        if (keys[k] != CLS_KEY_INVALID) atomicAdd(&s_h[keys[k] >> 15], 1u);
    }
    const int64_t mem_lo = c_lo + (int64_t)CB_REG_P * CB_THREADS;
    for (int64_t p = mem_lo + tid; p < c_hi; p += CB_THREADS) {
        const uint32_t key = cls_key(a, vc, pend_hi, w.sp, p);
        if (key != CLS_KEY_INVALID) atomicAdd(&s_h[key >> 15], 1u);
    }
    __syncthreads();
    // exclusive scan over the tiles, in place (thread t owns `per` consecutive tiles), and the workgroup's column of the table
    {
        const int per = (a.T + CB_THREADS - 1) / CB_THREADS;
        const int t0 = tid * per;
        const int gp = cls_table_pos(a, g);
        uint32_t sum = 0;
        for (int k = 0; k < per; ++k) sum += t0 + k < a.T ? s_h[t0 + k] : 0u;
        const int lane = tid & 63, wave = tid >> 6;
        const uint32_t inc = wave_incl_scan_add(sum);
        if (lane == 63) s_wsum[wave] = inc;
        __syncthreads();
        uint32_t run = inc - sum;
        for (int k = 0; k < wave; ++k) run += s_wsum[k];
        for (int k = 0; k < per; ++k) {
            const int t = t0 + k;
            if (t >= a.T) break;
            const uint32_t c = s_h[t];
            s_h[t] = run;
            a.table[(int64_t)t * a.Gr + gp] = make_uint2(c, run);
            run += c;
        }
    }
    __syncthreads();
    // pass B: one uint16_t per kept point into the workgroup's segment, by tile
    uint16_t *seg = a.recs + (int64_t)g * w.chunk;
#pragma unroll
    for (int k = 0; k < CB_REG_P; ++k) {
        if (keys[k] == CLS_KEY_INVALID) continue;
        const uint32_t pos = atomicAdd(&s_h[keys[k] >> 15], 1u);
        seg[pos] = (uint16_t)(keys[k] & 0x7fffu);
    }
    for (int64_t p = mem_lo + tid; p < c_hi; p += CB_THREADS) {
        const uint32_t key = cls_key(a, vc, pend_hi, w.sp, p);
        if (key == CLS_KEY_INVALID) continue;
        const uint32_t pos = atomicAdd(&s_h[key >> 15], 1u);
        seg[pos] = (uint16_t)(key & 0x7fffu);
    }
}

// ---------------------------------------------------------------------------------------------
// level 2
// ---------------------------------------------------------------------------------------------
#define CC_PLACES (CB_MAX_G + 8)                            // places of a table row at most
__global__ __launch_bounds__(CC_THREADS) void bev_class_cells(const ClsArgs a)
{
    __shared__ uint32_t s_cnt[2 * CC_TS * CC_TS * CC_MAX_S];  // [cell][set][group | all]
    __shared__ uint32_t s_bits[256];
    __shared__ uint32_t s_pre[CC_PLACES + 1];               // records of the tile in front of place p; [places] = all of them
    __shared__ uint32_t s_off[CC_PLACES];                   // where place p's run starts in the record buffer
    __shared__ uint32_t s_wsum[CC_THREADS / 64];
    const int tile = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int S = a.n_groups + 1;
    for (int i = tid; i < 2 * CC_TS * CC_TS * S; i += CC_THREADS) s_cnt[i] = 0;
    s_bits[tid] = a.cls_bits[tid];
    const int places = a.G > 0 ? a.Gr : 0;
    const int per = (places + CC_THREADS - 1) / CC_THREADS;
    uint32_t total = 0;
    if (places > 0) {
        const ClsWindow w = cls_window(a);
        const int p0 = tid * per;
        uint32_t cnt[(CC_PLACES + CC_THREADS - 1) / CC_THREADS];
        uint32_t sum = 0;
#pragma unroll
        for (int k = 0; k < (CC_PLACES + CC_THREADS - 1) / CC_THREADS; ++k) {
            const int p = p0 + k;
            cnt[k] = 0;
            if (k < per && p < places) {
                const int g = cls_table_group(a, p);
                if (g < a.G) {
                    const uint2 e = a.table[(int64_t)tile * a.Gr + p];
                    cnt[k] = e.x;
                    s_off[p] = (uint32_t)((int64_t)g * w.chunk) + e.y;
                }
            }
            sum += cnt[k];
        }
        const int lane = tid & 63, wave = tid >> 6;
        const uint32_t inc = wave_incl_scan_add(sum);
        if (lane == 63) s_wsum[wave] = inc;
        __syncthreads();
        uint32_t run = inc - sum;
        for (int k = 0; k < wave; ++k) run += s_wsum[k];
#pragma unroll
        for (int k = 0; k < (CC_PLACES + CC_THREADS - 1) / CC_THREADS; ++k) {
            const int p = p0 + k;
            if (k < per && p < places) s_pre[p] = run;
            run += cnt[k];
        }
        for (int k = 0; k < CC_THREADS / 64; ++k) total += s_wsum[k];
        if (tid == 0) s_pre[places] = total;
    }
    __syncthreads();
    // the tile's records: place by binary search over the prefix table, then one LDS atomic per group the class is in
    for (uint32_t r = tid; r < total; r += CC_THREADS) {
        int lo = 0, hi = places;                            // s_pre[lo] <= r < s_pre[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (s_pre[mid] <= r) lo = mid; else hi = mid;
        }
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
    const int px = a.prm.px, ng = a.n_groups;
    const int row0 = (tile / a.tx) * CC_TS, col0 = (tile % a.tx) * CC_TS;
    const size_t plane = (size_t)px * px;
    for (int i = tid; i < 3 * S * CC_TS * CC_TS; i += CC_THREADS) {
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
static inline int cls_tiles_x(int px) { return (px + CC_TS - 1) / CC_TS; }
// PCA_BEV_CLASS_G: a cap on level 1's workgroups, read on every call (tests set it to push chunks beyond the register path)
static inline int cls_level1_groups(int64_t max_points)
{
    const int max_g = (int)pca_env_int("PCA_BEV_CLASS_G", CB_MAX_G, 1, CB_MAX_G);
    const int64_t g = (max_points + CB_CHUNK - 1) / CB_CHUNK;
    return (int)(g < 1 ? 1 : (g > max_g ? max_g : g));
}
// The workspace: the records first (at the 256-byte aligned base), then the table.  The only place that knows the layout.
struct ClsLayout { int T, G, Gr, Gp; int64_t table, total; };
static ClsLayout cls_layout(int64_t max_points, int px)
{
    if (max_points < 1) max_points = 1;
    px = px < 1 ? 1 : (px > CLS_PX_MAX ? CLS_PX_MAX : px);
    ClsLayout l;
    const int tx = cls_tiles_x(px);
    l.T = tx * tx;
    l.G = cls_level1_groups(max_points);
    l.Gp = l.G >= 16 ? (l.G + 7) / 8 : 0;
    l.Gr = l.Gp ? 8 * l.Gp : l.G;
    l.table = pca_align256((max_points + l.G + 64) * 2);
    l.total = l.table + pca_align256((int64_t)l.T * l.Gr * 8) + 512;
    return l;
}

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
    if (!store || !frame_off || !prm || !groups || !workspace || (!prob && !prob_f16 && !counts)) {
        ctx->err = "bev class planes: bad arguments";
        return -1;
    }
    if (!store->x || !store->y || !store->z || !store->rgbs || !store->dyn) {
        ctx->err = "bev class planes: the store's x, y, z, rgbs and dyn arrays are needed";
        return -1;
    }
    if (prm->px < 1 || prm->px > CLS_PX_MAX) { ctx->err = "bev class planes: px must be in 1..1024"; return -1; }
    if (n_groups < 1 || n_groups > PCA_BEV_MAX_CLASS_GROUPS) { ctx->err = "bev class planes: n_groups must be in 1..16"; return -1; }
    if (!(prm->R[6] == 0.0 && prm->R[7] == 0.0 && prm->R[8] == 1.0 && prm->R[2] == 0.0 && prm->R[5] == 0.0)) {
        ctx->err = "bev class planes: R must be a rotation about the z axis (R[2] = R[5] = R[6] = R[7] = 0, R[8] = 1)";
        return -1;
    }
    if (!(slot_begin <= slot_split && slot_split <= slot_end)) {
        ctx->err = "bev class planes: need slot_begin <= slot_split <= slot_end";
        return -1;
    }
    if (n_pending < 0 || n_pending > PCA_BEV_MAX_CHAIN || (n_pending > 0 && (!pending_Ts || !pending_slot_ends))) {
        ctx->err = "bev class planes: bad chain of owed transforms";
        return -1;
    }
    if (max_points >= (1ll << 32) - 2 * CB_THREADS) { ctx->err = "bev class planes: window too large for 32-bit positions"; return -1; }
    const ClsLayout l = cls_layout(max_points, prm->px);
    if (workspace_bytes < l.total) { ctx->err = "bev class planes: workspace too small"; return -1; }
    ClsArgs A;
    A.st = *store;
    A.frame_off = frame_off;
    A.slot_begin = slot_begin; A.slot_split = slot_split; A.slot_end = slot_end;
    A.max_points = max_points;
    A.prm = *prm;
    A.n_pend = n_pending;
    for (int k = 0; k < PCA_BEV_MAX_CHAIN; ++k) {
        A.pend_slot_end[k] = slot_begin;
        for (int i = 0; i < 12; ++i) A.pend_T[k].m[i] = 0.0;
        if (k >= n_pending) continue;
        if (pending_slot_ends[k] > slot_end) { ctx->err = "bev class planes: a pending slot end lies beyond the window"; return -1; }
        if (k > 0 && pending_slot_ends[k] < pending_slot_ends[k - 1]) { ctx->err = "bev class planes: pending slot ends must ascend"; return -1; }
        A.pend_slot_end[k] = pending_slot_ends[k];
        for (int i = 0; i < 12; ++i) A.pend_T[k].m[i] = pending_Ts[16 * k + i];
    }
    A.tx = cls_tiles_x(prm->px);
    A.T = l.T;
    A.G = slot_end > slot_begin ? l.G : 0;                  // a window without a slot: no launch over zero points
    A.Gr = l.Gr; A.Gp = l.Gp;
    A.n_groups = n_groups;
    char *w = reinterpret_cast<char *>(pca_align256(reinterpret_cast<intptr_t>(workspace)));
    A.recs = reinterpret_cast<uint16_t *>(w);
    A.table = reinterpret_cast<uint2 *>(w + l.table);
    A.prob = prob; A.prob_f16 = prob_f16; A.counts = counts;
    A.status = ctx->ticket + 1;
    for (int c = 0; c < 256; ++c) {
        uint32_t bits = 1u << n_groups;
        for (int g = 0; g < n_groups; ++g) bits |= (uint32_t)((groups[g].mask[c >> 6] >> (c & 63)) & 1ull) << g;
        A.cls_bits[c] = bits;
    }
    PCA_CHECK(ctx, hipSetDevice(ctx->device));
    if (pca_k1_flush_pending(ctx)) return -1;               // a noted K1 runs on its own first, as before a banded raster
    static bool lds_set = false;                            // level 1's histogram is 64 KiB of dynamic LDS at 1024^2
    if (!lds_set) {
        PCA_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(bev_class_bin), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (CLS_PX_MAX / CC_TS) * (CLS_PX_MAX / CC_TS) * 4));
        lds_set = true;
    }
    const ClsArgs &args = A;
    if (args.G > 0)
        PCA_LAUNCH_SHM(ctx, PCA_K_BEV_CLASS_BIN, bev_class_bin, dim3(args.G), dim3(CB_THREADS), (size_t)args.T * 4, s, args);
    PCA_LAUNCH(ctx, PCA_K_BEV_CLASS_CELLS, bev_class_cells, dim3(args.T), dim3(CC_THREADS), s, args);
    PCA_CHECK(ctx, hipGetLastError());
    return 0;
}

}  // extern "C"
