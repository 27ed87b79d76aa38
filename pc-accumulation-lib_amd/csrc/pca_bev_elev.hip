// pca_bev_elev.hip -- the BEV window partitioned by height above the cell minimum: two passes over the window for gfx950.
//
// The reference's SemBEVGenerator.static_obj_partitioning_by_elev (bev_generator/sem_bev.py:556-591) builds the per-cell
// minimum-z map of the rows it is given and flags every row whose z lies more than elev_thresh above its cell's minimum: two
// per-point Python loops.  Here pass one is a cell minimum and pass two compares each point with its cell, with the
// structure of the class planes (pca_bev_class.hip): two levels, LDS atomics only, no global atomics.
//
//   level 1  bev_elev_bin      1024 threads; workgroup g takes chunk g of the window: owed re-transforms, view test and cell
//                              exactly as cls_key of pca_bev_class.hip / view_key of pca_bev.hip spell them out -> key =
//                              tile << 6 | cell_in_tile; LDS histogram over the 8x8-cell tiles (4 B per tile: 64 KiB at 1024^2);
//                              exclusive scan IN PLACE (the histogram becomes the cursors); the kept points' records --
//                              {z in the BEV frame f64, index in the window u32, cell_in_tile u32}, 16 bytes -- sorted by tile
//                              into the workgroup's own segment; {count, offset} per (tile, workgroup) into the table.  A
//                              point that is NOT kept gets flags[index] = 255 here (coalesced).  The first EB_REG_P x 1024
//                              points of a chunk keep key and z in registers between the passes; what a chunk holds beyond
//                              that is recomputed from L2.
//   level 2  bev_elev_cells    256 threads, one workgroup per tile: prefix table over the workgroups' runs in LDS, binary
//                              search per record; pass A: LDS minimum per cell over the order-preserving u64 key of z (the
//                              main raster's elevation plane), barrier, pass B: elevated = z > (min + elev_thresh) as an f64
//                              add and an f64 compare, flags[index] = elevated; counts per tile in LDS; whole tile rows of
//                              `elev` and `observed`; three int64 words per tile for the totals.
//   tail     bev_elev_totals   one workgroup: the per-tile words summed into counts[3] (no global atomics).
// Every byte of flags[0, n) is written exactly once per call: by level 1 (255) or by level 2 (0 / 1).
// The order in which a tile's records arrive is not fixed (LDS cursors); neither the minimum nor a flag depends on it.
#include "pca_bev_common.h"

#define EB_THREADS 1024           // workgroup size of level 1
#define EB_REG_P 12               // points per thread of level 1 whose key and z stay in registers between its passes
#define EB_MAX_G 512              // workgroups of level 1 at most (two rounds of one per CU)
#define EB_CHUNK 8192             // points per workgroup of level 1 the launch is sized for
#define EC_THREADS 256            // workgroup size of level 2
#define EC_TS 8                   // tile side [cells]
#define ET_THREADS 1024           // workgroup size of the tail
#define ELV_PX_MAX 1024
#define ELV_KEY_INVALID 0xffffffffu

struct alignas(16) ElvRec { double z; uint32_t idx, cell; };

struct alignas(16) ElvArgs {
    pca_store st;
    const int64_t *frame_off;
    int slot_begin, slot_end;
    int64_t max_points;
    pca_bev_params prm;
    double thresh;
    int include_dyn;
    int n_pend;                   // owed re-transforms, oldest first: transform k is owed by slots [slot_begin, pend_slot_end[k])
    int pend_slot_end[PCA_BEV_MAX_CHAIN];
    Mat34 pend_T[PCA_BEV_MAX_CHAIN];
    int tx, T;                    // tiles per row, tiles
    int G;                        // workgroups of level 1; 0: the window holds no slot, level 2 alone writes the empty maps
    int Gr, Gp;                   // the table's row length (>= G) and workgroups per XCD column block (elv_table_pos)
    ElvRec *recs;                 // [max_points + G], tile-ordered per segment
    uint2 *table;                 // [T][Gr] {kept records, offset in the segment} per (tile, workgroup)
    int64_t *tile_counts;         // [3][T]: in view, elevated, not elevated
    double *elev;                 // [px][px] or NULL
    uint8_t *observed;            // [px][px] or NULL
    uint8_t *flags;               // [window points] or NULL
    int64_t *counts;              // [3] or NULL
    uint32_t *status;             // context status word (PCA_STATUS_* bits)
};

struct ElvWindow { int64_t lo, hi, chunk; };
// the window as both kernels see it (frame_off lives on the device); above max_points it is cut, as the main raster cuts it
__device__ __forceinline__ ElvWindow elv_window(const ElvArgs &a)
{
    ElvWindow w;
    w.lo = a.frame_off[a.slot_begin];
    const int64_t hi0 = a.frame_off[a.slot_end];
    w.hi = (hi0 - w.lo > a.max_points) ? w.lo + a.max_points : hi0;
    const int G = a.G > 0 ? a.G : 1;
    w.chunk = (w.hi - w.lo + G - 1) / G;
    return w;
}
// The table is [tile][Gr] with workgroup g at position (g mod 8) Gp + g / 8, as the class planes' table is.  Gp = 0: plain order.
__device__ __forceinline__ int elv_table_pos(const ElvArgs &a, int g) { return a.Gp ? (g & 7) * a.Gp + (g >> 3) : g; }
__device__ __forceinline__ int elv_table_group(const ElvArgs &a, int p)
{
    if (!a.Gp) return p;
    const int x = p / a.Gp;
    return (p - x * a.Gp) * 8 + x;                          // may be >= G: an unused place of the row
}

// The view test and the cell of one point, the main raster's (view_key of pca_bev.hip; R is a rotation about z, checked by
// the host, so R[2] z, R[5] z, R[6] x and R[7] y are exact zeros and R[8] z is z for finite z; a point whose z is not finite
// is dropped, as the reference drops it: 0 * inf = NaN poisons its x and y).
struct ElvView { double ox, oy, oz, r0, r1, r3, r4, dx, dy, vlo, vhi, v, rv, pxd, half_px, hf; int px, tx; bool use_h, all_dyn; };
__device__ __forceinline__ ElvView elv_view(const ElvArgs &a)
{
    const pca_bev_params &q = a.prm;
    ElvView c;
    c.ox = q.origin[0]; c.oy = q.origin[1]; c.oz = q.origin[2];
    c.r0 = q.R[0]; c.r1 = q.R[1]; c.r3 = q.R[3]; c.r4 = q.R[4];
    c.dx = q.dx; c.dy = q.dy;
    c.v = q.view; c.rv = 1.0 / q.view; c.vlo = -0.5 * q.view; c.vhi = 0.5 * q.view; c.pxd = (double)q.px; c.half_px = 0.5 * c.pxd;
    c.hf = q.height_filter; c.use_h = !(q.height_filter != q.height_filter);
    c.px = q.px; c.tx = a.tx;
    c.all_dyn = a.include_dyn != 0;
    return c;
}
struct ElvPendHi { int64_t v[PCA_BEV_MAX_CHAIN]; };         // first point index that does NOT owe transform k
// the owed re-transforms of point p, oldest first, each a separate fma chain (the roundings of one K2 pass per transform)
__device__ __forceinline__ void elv_apply_owed(const ElvArgs &a, const ElvPendHi &pend_hi, int64_t p, double &X, double &Y, double &Z)
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
// key of stored point p: tile << 6 | cell_in_tile, ELV_KEY_INVALID = not in view; z: its height in the BEV frame
__device__ __forceinline__ uint32_t elv_key(const ElvArgs &a, const ElvView &c, const ElvPendHi &pend_hi, int64_t p, double &z)
{
    double X = pca_ldg(a.st.x + p), Y = pca_ldg(a.st.y + p), Z = pca_ldg(a.st.z + p);
    const uint8_t D = pca_ldg(a.st.dyn + p);
    elv_apply_owed(a, pend_hi, p, X, Y, Z);
    const double x = X - c.ox, y = Y - c.oy;
    const double ax = fma(c.r1, y, c.r0 * x) + c.dx;
    const double ay = fma(c.r4, y, c.r3 * x) + c.dy;
    bool keep = (c.all_dyn || D != 1) && (ax > c.vlo) && (ax < c.vhi) && (ay > c.vlo) && (ay < c.vhi) && (fabs(Z) < __builtin_huge_val());
    if (c.use_h) keep = keep && (Z - c.oz < c.hf);
    z = (Z - c.oz) + 0.0;                                   // (the reference's matmul turns a z of -0.0 into +0.0)
    if (!keep) return ELV_KEY_INVALID;
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
    const uint32_t tile = (row / EC_TS) * (uint32_t)c.tx + col / EC_TS;
    const uint32_t cell = (row % EC_TS) * EC_TS + col % EC_TS;
    return (tile << 6) | cell;
}
__device__ __forceinline__ void elv_store_rec(ElvRec *dst, double z, uint32_t idx, uint32_t cell)
{
    const uint64_t zb = (uint64_t)__double_as_longlong(z);
    *reinterpret_cast<uint4 *>(dst) = make_uint4((uint32_t)zb, (uint32_t)(zb >> 32), idx, cell);   // one 16-byte store
}

// ---------------------------------------------------------------------------------------------
// level 1
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EB_THREADS) void bev_elev_bin(const ElvArgs a)
{
    extern __shared__ uint32_t s_h[];                       // [T]: histogram over the tiles, after the scan the cursors
    __shared__ uint32_t s_wsum[EB_THREADS / 64];
    const int g = (int)blockIdx.x, tid = (int)threadIdx.x;
    const ElvWindow w = elv_window(a);
    int64_t c_lo = w.lo + (int64_t)g * w.chunk;
    int64_t c_hi = c_lo + w.chunk < w.hi ? c_lo + w.chunk : w.hi;
    if (c_lo > w.hi) c_lo = c_hi = w.hi;
    if (g == 0 && tid == 0 && a.frame_off[a.slot_end] - w.lo > a.max_points) pca_raise(a.status, PCA_STATUS_STORE_OVERFLOW);
    for (int t = tid; t < a.T; t += EB_THREADS) s_h[t] = 0;
    __syncthreads();
    ElvPendHi pend_hi;
#pragma unroll
    for (int k = 0; k < PCA_BEV_MAX_CHAIN; ++k)
        pend_hi.v[k] = (k < a.n_pend && a.pend_slot_end[k] > a.slot_begin) ? a.frame_off[a.pend_slot_end[k]] : w.lo;
    const ElvView vc = elv_view(a);
    // pass A: keys, the histogram and the flag of every point that is not kept
    uint32_t keys[EB_REG_P];
    double zs[EB_REG_P];
#pragma unroll
    for (int k = 0; k < EB_REG_P; ++k) {
        const int64_t p = c_lo + (int64_t)k * EB_THREADS + tid;
        keys[k] = ELV_KEY_INVALID;
        zs[k] = 0.0;
        if (p < c_hi) {
            keys[k] = elv_key(a, vc, pend_hi, p, zs[k]);
            if (keys[k] != ELV_KEY_INVALID) atomicAdd(&s_h[keys[k] >> 6], 1u);
            else if (a.flags) a.flags[p - w.lo] = 255;
        }
    }
    const int64_t mem_lo = c_lo + (int64_t)EB_REG_P * EB_THREADS;
    for (int64_t p = mem_lo + tid; p < c_hi; p += EB_THREADS) {
        double z;
        const uint32_t key = elv_key(a, vc, pend_hi, p, z);
        if (key != ELV_KEY_INVALID) atomicAdd(&s_h[key >> 6], 1u);
        else if (a.flags) a.flags[p - w.lo] = 255;
    }
    __syncthreads();
    // exclusive scan over the tiles, in place (thread t owns `per` consecutive tiles), and the workgroup's column of the table
    {
        const int per = (a.T + EB_THREADS - 1) / EB_THREADS;
        const int t0 = tid * per;
        const int gp = elv_table_pos(a, g);
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
    // pass B: one 16-byte record per kept point into the workgroup's segment, by tile
    ElvRec *seg = a.recs + (int64_t)g * w.chunk;
#pragma unroll
    for (int k = 0; k < EB_REG_P; ++k) {
        if (keys[k] == ELV_KEY_INVALID) continue;
        const int64_t p = c_lo + (int64_t)k * EB_THREADS + tid;
        const uint32_t pos = atomicAdd(&s_h[keys[k] >> 6], 1u);
        elv_store_rec(seg + pos, zs[k], (uint32_t)(p - w.lo), keys[k] & 63u);
    }
    for (int64_t p = mem_lo + tid; p < c_hi; p += EB_THREADS) {
        double z;
        const uint32_t key = elv_key(a, vc, pend_hi, p, z);
        if (key == ELV_KEY_INVALID) continue;
        const uint32_t pos = atomicAdd(&s_h[key >> 6], 1u);
        elv_store_rec(seg + pos, z, (uint32_t)(p - w.lo), key & 63u);
    }
}

// ---------------------------------------------------------------------------------------------
// level 2
// ---------------------------------------------------------------------------------------------
#define EC_PLACES (EB_MAX_G + 8)                            // places of a table row at most
// the r-th record of the tile: its place by binary search over the prefix table
__device__ __forceinline__ uint4 elv_load_rec(const ElvArgs &a, const uint32_t *s_pre, const uint32_t *s_off, int places, uint32_t r)
{
    int lo = 0, hi = places;                                // s_pre[lo] <= r < s_pre[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (s_pre[mid] <= r) lo = mid; else hi = mid;
    }
    return *reinterpret_cast<const uint4 *>(a.recs + ((size_t)s_off[lo] + (r - s_pre[lo])));
}
__global__ __launch_bounds__(EC_THREADS) void bev_elev_cells(const ElvArgs a)
{
    __shared__ unsigned long long s_min[EC_TS * EC_TS];     // order key of the cell's minimum z, ~0 = no record
    __shared__ uint32_t s_pre[EC_PLACES + 1];               // records of the tile in front of place p; [places] = all of them
    __shared__ uint32_t s_off[EC_PLACES];                   // where place p's run starts in the record buffer
    __shared__ uint32_t s_wsum[EC_THREADS / 64];
    __shared__ uint32_t s_elevated;
    const int tile = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (tid < EC_TS * EC_TS) s_min[tid] = ~0ull;
    if (tid == 0) s_elevated = 0;
    const int places = a.G > 0 ? a.Gr : 0;
    const int per = (places + EC_THREADS - 1) / EC_THREADS;
    uint32_t total = 0;
    if (places > 0) {
        const ElvWindow w = elv_window(a);
        const int p0 = tid * per;
        uint32_t cnt[(EC_PLACES + EC_THREADS - 1) / EC_THREADS];
        uint32_t sum = 0;
#pragma unroll
        for (int k = 0; k < (EC_PLACES + EC_THREADS - 1) / EC_THREADS; ++k) {
            const int p = p0 + k;
            cnt[k] = 0;
            if (k < per && p < places) {
                const int g = elv_table_group(a, p);
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
        for (int k = 0; k < (EC_PLACES + EC_THREADS - 1) / EC_THREADS; ++k) {
            const int p = p0 + k;
            if (k < per && p < places) s_pre[p] = run;
            run += cnt[k];
        }
        for (int k = 0; k < EC_THREADS / 64; ++k) total += s_wsum[k];
        if (tid == 0) s_pre[places] = total;
    }
    __syncthreads();
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
    const int px = a.prm.px;
    const int row0 = (tile / a.tx) * EC_TS, col0 = (tile % a.tx) * EC_TS;
    if (tid < EC_TS * EC_TS) {
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
        a.tile_counts[(size_t)a.T + tile] = e;
        a.tile_counts[2 * (size_t)a.T + tile] = (int64_t)total - e;
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
        for (int t = tid; t < a.T; t += ET_THREADS) v += (unsigned long long)a.tile_counts[(size_t)q * a.T + t];
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
static inline int elv_tiles_x(int px) { return (px + EC_TS - 1) / EC_TS; }
// PCA_BEV_ELEV_G: a cap on level 1's workgroups, read on every call (tests set it to push chunks beyond the register path)
static inline int elv_level1_groups(int64_t max_points)
{
    const int max_g = (int)pca_env_int("PCA_BEV_ELEV_G", EB_MAX_G, 1, EB_MAX_G);
    const int64_t g = (max_points + EB_CHUNK - 1) / EB_CHUNK;
    return (int)(g < 1 ? 1 : (g > max_g ? max_g : g));
}
// The workspace: the records first (at the 256-byte aligned base), then the table, then the per-tile totals.  The only place
// that knows the layout.
struct ElvLayout { int T, G, Gr, Gp; int64_t table, tile_counts, total; };
static ElvLayout elv_layout(int64_t max_points, int px)
{
    if (max_points < 1) max_points = 1;
    px = px < 1 ? 1 : (px > ELV_PX_MAX ? ELV_PX_MAX : px);
    ElvLayout l;
    const int tx = elv_tiles_x(px);
    l.T = tx * tx;
    l.G = elv_level1_groups(max_points);
    l.Gp = l.G >= 16 ? (l.G + 7) / 8 : 0;
    l.Gr = l.Gp ? 8 * l.Gp : l.G;
    l.table = pca_align256((max_points + l.G + 64) * (int64_t)sizeof(ElvRec));
    l.tile_counts = l.table + pca_align256((int64_t)l.T * l.Gr * 8);
    l.total = l.tile_counts + pca_align256((int64_t)l.T * 3 * 8) + 512;
    return l;
}

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
    if (!store || !frame_off || !prm || !workspace || (!elev && !observed && !flags && !counts)) {
        ctx->err = "bev elev partition: bad arguments";
        return -1;
    }
    if (!store->x || !store->y || !store->z || !store->dyn) {
        ctx->err = "bev elev partition: the store's x, y, z and dyn arrays are needed";
        return -1;
    }
    if (elev_thresh != elev_thresh) { ctx->err = "bev elev partition: elev_thresh is NaN"; return -1; }
    if (prm->px < 1 || prm->px > ELV_PX_MAX) { ctx->err = "bev elev partition: px must be in 1..1024"; return -1; }
    if (!(prm->R[6] == 0.0 && prm->R[7] == 0.0 && prm->R[8] == 1.0 && prm->R[2] == 0.0 && prm->R[5] == 0.0)) {
        ctx->err = "bev elev partition: R must be a rotation about the z axis (R[2] = R[5] = R[6] = R[7] = 0, R[8] = 1)";
        return -1;
    }
    if (slot_begin > slot_end) { ctx->err = "bev elev partition: need slot_begin <= slot_end"; return -1; }
    if (n_pending < 0 || n_pending > PCA_BEV_MAX_CHAIN || (n_pending > 0 && (!pending_Ts || !pending_slot_ends))) {
        ctx->err = "bev elev partition: bad chain of owed transforms";
        return -1;
    }
    if (max_points >= (1ll << 32) - 2 * EB_THREADS) { ctx->err = "bev elev partition: window too large for 32-bit positions"; return -1; }
    const ElvLayout l = elv_layout(max_points, prm->px);
    if (workspace_bytes < l.total) { ctx->err = "bev elev partition: workspace too small"; return -1; }
    ElvArgs A;
    A.st = *store;
    A.frame_off = frame_off;
    A.slot_begin = slot_begin; A.slot_end = slot_end;
    A.max_points = max_points;
    A.prm = *prm;
    A.thresh = elev_thresh;
    A.include_dyn = include_dyn;
    A.n_pend = n_pending;
    for (int k = 0; k < PCA_BEV_MAX_CHAIN; ++k) {
        A.pend_slot_end[k] = slot_begin;
        for (int i = 0; i < 12; ++i) A.pend_T[k].m[i] = 0.0;
        if (k >= n_pending) continue;
        if (pending_slot_ends[k] > slot_end) { ctx->err = "bev elev partition: a pending slot end lies beyond the window"; return -1; }
        if (k > 0 && pending_slot_ends[k] < pending_slot_ends[k - 1]) { ctx->err = "bev elev partition: pending slot ends must ascend"; return -1; }
        A.pend_slot_end[k] = pending_slot_ends[k];
        for (int i = 0; i < 12; ++i) A.pend_T[k].m[i] = pending_Ts[16 * k + i];
    }
    A.tx = elv_tiles_x(prm->px);
    A.T = l.T;
    A.G = slot_end > slot_begin ? l.G : 0;                  // a window without a slot: no launch over zero points
    A.Gr = l.Gr; A.Gp = l.Gp;
    char *w = reinterpret_cast<char *>(pca_align256(reinterpret_cast<intptr_t>(workspace)));
    A.recs = reinterpret_cast<ElvRec *>(w);
    A.table = reinterpret_cast<uint2 *>(w + l.table);
    A.tile_counts = reinterpret_cast<int64_t *>(w + l.tile_counts);
    A.elev = elev; A.observed = observed; A.flags = flags; A.counts = counts;
    A.status = ctx->ticket + 1;
    PCA_CHECK(ctx, hipSetDevice(ctx->device));
    if (pca_k1_flush_pending(ctx)) return -1;               // a noted K1 runs on its own first, as before the class planes
    static bool lds_set = false;                            // level 1's histogram is 64 KiB of dynamic LDS at 1024^2
    if (!lds_set) {
        PCA_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(bev_elev_bin), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (ELV_PX_MAX / EC_TS) * (ELV_PX_MAX / EC_TS) * 4));
        lds_set = true;
    }
    const ElvArgs &args = A;
    if (args.G > 0)
        PCA_LAUNCH_SHM(ctx, PCA_K_BEV_ELEV_BIN, bev_elev_bin, dim3(args.G), dim3(EB_THREADS), (size_t)args.T * 4, s, args);
    PCA_LAUNCH(ctx, PCA_K_BEV_ELEV_CELLS, bev_elev_cells, dim3(args.T), dim3(EC_THREADS), s, args);
    if (args.counts) PCA_LAUNCH(ctx, PCA_K_BEV_ELEV_CELLS, bev_elev_totals, dim3(1), dim3(ET_THREADS), s, args);
    PCA_CHECK(ctx, hipGetLastError());
    return 0;
}

}  // extern "C"
