// pca_bev_side.h -- the scaffold of the side passes over the BEV window (the class planes pca_bev_class.hip, the elevation
// partition pca_bev_elev.hip, the occupancy labels pca_bev_voxel.hip): two levels, LDS atomics only, no global atomics.
//
//   level 1  side_bin<Policy>  1024 threads; workgroup g takes chunk g of the window: the policy's key of every point (owed
//                              re-transforms, view test and cell: pca_bev_view.h), tile in the key's high bits; LDS histogram
//                              over the 8x8-cell tiles (4 B per tile: 64 KiB at 1024^2); exclusive scan IN PLACE (the histogram
//                              becomes the cursors); the kept points' records sorted by tile into the workgroup's own segment;
//                              {count, offset} per (tile, workgroup) into the table.  The first REG_P x 1024 points of a chunk
//                              keep key and payload in registers between the passes (a 200-frame KITTI window: all of it);
//                              what a chunk holds beyond that is recomputed from L2.
//   level 2  side_tile_runs    256 threads, one workgroup per tile: prefix table over the workgroups' runs in LDS; side_find:
//                              binary search per record.  What a pass does with its records is its own.
// The order in which a tile's records arrive is not fixed (LDS cursors); neither pass's results depend on it.
#pragma once
#include "pca_bev_view.h"

#define SIDE_BIN_THREADS 1024     // workgroup size of level 1
#define SIDE_MAX_G 512            // workgroups of level 1 at most (two rounds of one per CU)
#define SIDE_CHUNK 8192           // points per workgroup of level 1 the launch is sized for
#define SIDE_CELLS_THREADS 256    // workgroup size of level 2
#define SIDE_PLACES (SIDE_MAX_G + 8)   // places of a table row at most

struct SideArgs {                 // the first member of every pass's argument block
    pca_store st;
    const int64_t *frame_off;
    int slot_begin, slot_split, slot_end;
    int64_t max_points;
    pca_bev_params prm;
    BevOwed owed;                 // owed re-transforms: applied to what the pass reads, never written back
    int tx, T;                    // tiles per row, tiles
    int G;                        // workgroups of level 1; 0: the window holds no slot, level 2 alone writes the empty maps
    int Gr, Gp;                   // the table's row length (>= G) and workgroups per XCD column block (bev_table_pos)
    uint2 *table;                 // [T][Gr] {kept records, offset in the segment} per (tile, workgroup)
    uint32_t *status;             // context status word (PCA_STATUS_* bits)
};

struct SideWindow { int64_t lo, hi, sp, chunk; };
// the window as both levels see it (frame_off lives on the device); above max_points it is cut, as the main raster cuts it
__device__ __forceinline__ SideWindow side_window(const SideArgs &a)
{
    SideWindow w;
    w.lo = a.frame_off[a.slot_begin];
    const int64_t hi0 = a.frame_off[a.slot_end];
    w.sp = a.frame_off[a.slot_split];
    w.hi = (hi0 - w.lo > a.max_points) ? w.lo + a.max_points : hi0;
    const int G = a.G > 0 ? a.G : 1;
    w.chunk = (w.hi - w.lo + G - 1) / G;
    return w;
}

// Level 1.  The policy supplies
//   REG_P, SHIFT           points per thread kept in registers; key >> SHIFT = the tile
//   Payload                what a kept point carries beside its key between the passes
//   key(a, vc, pend_hi, w, p, payload) -> the key of stored point p, KEY_INVALID = dropped
//   dropped(w, p)          a point of the window that is not kept (pass A)
//   store(g, w, pos, key, payload, p)   the record of a kept point at position `pos` of workgroup g's segment (pass B)
template <typename Policy>
__device__ __forceinline__ void side_bin(const SideArgs &a, const Policy pol)
{
    constexpr int REG_P = Policy::REG_P, SHIFT = Policy::SHIFT;
    extern __shared__ uint32_t s_h[];                       // [T]: histogram over the tiles, after the scan the cursors
    __shared__ uint32_t s_wsum[SIDE_BIN_THREADS / 64];
    const int g = (int)blockIdx.x, tid = (int)threadIdx.x;
    const SideWindow w = side_window(a);
    int64_t c_lo = w.lo + (int64_t)g * w.chunk;
    int64_t c_hi = c_lo + w.chunk < w.hi ? c_lo + w.chunk : w.hi;
    if (c_lo > w.hi) c_lo = c_hi = w.hi;
    if (g == 0 && tid == 0 && a.frame_off[a.slot_end] - w.lo > a.max_points) pca_raise(a.status, PCA_STATUS_STORE_OVERFLOW);
    for (int t = tid; t < a.T; t += SIDE_BIN_THREADS) s_h[t] = 0;
    __syncthreads();
    const PendHi pend_hi = owed_bounds(a.owed, a.frame_off, a.slot_begin, w.lo);
    const ViewConst vc = view_const(a.prm, a.tx, 0, 0);
    // pass A: keys, the histogram and what the policy does with a point that is not kept
    uint32_t keys[REG_P];
    typename Policy::Payload pay[REG_P];
#pragma unroll
    for (int k = 0; k < REG_P; ++k) {
        const int64_t p = c_lo + (int64_t)k * SIDE_BIN_THREADS + tid;
        keys[k] = KEY_INVALID;
        pay[k] = typename Policy::Payload();
        if (p < c_hi) {
            keys[k] = pol.key(a, vc, pend_hi, w, p, pay[k]);
            if (keys[k] != KEY_INVALID) atomicAdd(&s_h[keys[k] >> SHIFT], 1u);
            else pol.dropped(w, p);
        }
    }
    const int64_t mem_lo = c_lo + (int64_t)REG_P * SIDE_BIN_THREADS;
    for (int64_t p = mem_lo + tid; p < c_hi; p += SIDE_BIN_THREADS) {
        typename Policy::Payload pl;
        const uint32_t key = pol.key(a, vc, pend_hi, w, p, pl);
        if (key != KEY_INVALID) atomicAdd(&s_h[key >> SHIFT], 1u);
        else pol.dropped(w, p);
    }
    __syncthreads();
    // exclusive scan over the tiles, in place (thread t owns `per` consecutive tiles), and the workgroup's column of the table
    {
        const int per = (a.T + SIDE_BIN_THREADS - 1) / SIDE_BIN_THREADS;
        const int t0 = tid * per;
        const int gp = bev_table_pos(a.Gp, g);
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
    // pass B: one record per kept point into the workgroup's segment, by tile
#pragma unroll
    for (int k = 0; k < REG_P; ++k) {
        if (keys[k] == KEY_INVALID) continue;
        const int64_t p = c_lo + (int64_t)k * SIDE_BIN_THREADS + tid;
        const uint32_t pos = atomicAdd(&s_h[keys[k] >> SHIFT], 1u);
        pol.store(g, w, pos, keys[k], pay[k], p);
    }
    for (int64_t p = mem_lo + tid; p < c_hi; p += SIDE_BIN_THREADS) {
        typename Policy::Payload pl;
        const uint32_t key = pol.key(a, vc, pend_hi, w, p, pl);
        if (key == KEY_INVALID) continue;
        const uint32_t pos = atomicAdd(&s_h[key >> SHIFT], 1u);
        pol.store(g, w, pos, key, pl, p);
    }
}

// Level 2, all SIDE_CELLS_THREADS threads: the runs of `tile` in the workgroups' segments.  s_pre[p] = records of the tile in
// front of place p of its table row, s_pre[places] = all of them (returned); s_off[p] = where place p's run starts in the
// record buffer.  Ends with a barrier (which also publishes what the caller initialised in LDS before the call).
__device__ __forceinline__ uint32_t side_tile_runs(const SideArgs &a, int tile, uint32_t *s_pre, uint32_t *s_off, uint32_t *s_wsum, int &places)
{
    constexpr int PER_MAX = (SIDE_PLACES + SIDE_CELLS_THREADS - 1) / SIDE_CELLS_THREADS;
    const int tid = (int)threadIdx.x;
    places = a.G > 0 ? a.Gr : 0;
    const int per = (places + SIDE_CELLS_THREADS - 1) / SIDE_CELLS_THREADS;
    uint32_t total = 0;
    if (places > 0) {
        const SideWindow w = side_window(a);
        const int p0 = tid * per;
        uint32_t cnt[PER_MAX];
        uint32_t sum = 0;
#pragma unroll
        for (int k = 0; k < PER_MAX; ++k) {
            const int p = p0 + k;
            cnt[k] = 0;
            if (k < per && p < places) {
                const int g = bev_table_group(a.Gp, p);
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
        for (int k = 0; k < PER_MAX; ++k) {
            const int p = p0 + k;
            if (k < per && p < places) s_pre[p] = run;
            run += cnt[k];
        }
        for (int k = 0; k < SIDE_CELLS_THREADS / 64; ++k) total += s_wsum[k];
        if (tid == 0) s_pre[places] = total;
    }
    __syncthreads();
    return total;
}
// the place that holds the tile's r-th record: s_pre[place] <= r < s_pre[place + 1]
__device__ __forceinline__ int side_find(const uint32_t *s_pre, int places, uint32_t r)
{
    int lo = 0, hi = places;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (s_pre[mid] <= r) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- host side ----
static inline int side_tiles_x(int px) { return (px + TS - 1) / TS; }
// env_name (PCA_BEV_CLASS_G / PCA_BEV_ELEV_G / PCA_BEV_VOXEL_G): a cap on level 1's workgroups, read on every call (tests set
// it to push chunks beyond the register path)
static inline int side_groups(int64_t max_points, const char *env_name)
{
    const int max_g = (int)pca_env_int(env_name, SIDE_MAX_G, 1, SIDE_MAX_G);
    const int64_t g = (max_points + SIDE_CHUNK - 1) / SIDE_CHUNK;
    return (int)(g < 1 ? 1 : (g > max_g ? max_g : g));
}
// The workspace: the records first (at the 256-byte aligned base), then the table, then tile_bytes per tile of the pass's own.
// The only place that knows the layout.
struct SideLayout { int T, G, Gr, Gp; int64_t table, tail, total; };
static inline SideLayout side_layout(int64_t max_points, int px, int64_t record_bytes, int64_t tile_bytes, const char *env_name)
{
    if (max_points < 1) max_points = 1;
    px = px < 1 ? 1 : (px > SIDE_PX_MAX ? SIDE_PX_MAX : px);
    SideLayout l;
    const int tx = side_tiles_x(px);
    l.T = tx * tx;
    l.G = side_groups(max_points, env_name);
    l.Gp = l.G >= 16 ? (l.G + 7) / 8 : 0;
    l.Gr = l.Gp ? 8 * l.Gp : l.G;
    l.table = pca_align256((max_points + l.G + 64) * record_bytes);
    l.tail = l.table + pca_align256((int64_t)l.T * l.Gr * 8);
    l.total = l.tail + pca_align256((int64_t)l.T * tile_bytes) + 512;
    return l;
}
// The tiled passes' part of the checks, after window_check (pca_bev_view.h) has filled A's window: the tiles, the table and
// the workspace; l: the pass's layout for (A.max_points, A.prm.px); `base`: the 256-byte aligned workspace its offsets count from.
static inline int side_tiles(pca_ctx *ctx, const char *what, int slot_split, void *workspace, int64_t workspace_bytes,
                             const SideLayout &l, SideArgs &A, char *&base)
{
    const std::string w(what);
    if (A.max_points >= (1ll << 32) - 2 * SIDE_BIN_THREADS) { ctx->err = w + ": window too large for 32-bit positions"; return -1; }
    if (workspace_bytes < l.total) { ctx->err = w + ": workspace too small"; return -1; }
    A.slot_split = slot_split;
    A.tx = side_tiles_x(A.prm.px);
    A.T = l.T;
    A.G = A.slot_end > A.slot_begin ? l.G : 0;              // a window without a slot: no launch over zero points
    A.Gr = l.Gr; A.Gp = l.Gp;
    base = reinterpret_cast<char *>(pca_align256(reinterpret_cast<intptr_t>(workspace)));
    A.table = reinterpret_cast<uint2 *>(base + l.table);
    return 0;
}
// level 1's histogram is 64 KiB of dynamic LDS at 1024^2: asked for once per process and kernel
template <auto KERNEL>
static int side_grant_lds(pca_ctx *ctx)
{
    static bool lds_set = false;
    if (lds_set) return 0;
    PCA_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (SIDE_PX_MAX / TS) * (SIDE_PX_MAX / TS) * 4));
    lds_set = true;
    return 0;
}
// The launch tail the tiled passes share: the device, a noted K1 on its own first (as before a banded raster), level 1's LDS
// and level 1 itself -- unless the window holds no slot.  Args: the pass's argument block, SideArgs first.
template <auto BIN, typename Args>
static int side_launch_bin(pca_ctx *ctx, int kernel_id, const Args &args, hipStream_t s)
{
    PCA_CHECK(ctx, hipSetDevice(ctx->device));
    if (pca_k1_flush_pending(ctx)) return -1;
    if (side_grant_lds<BIN>(ctx)) return -1;
    if (args.s.G > 0)
        PCA_LAUNCH_SHM(ctx, kernel_id, BIN, dim3(args.s.G), dim3(SIDE_BIN_THREADS), (size_t)args.s.T * 4, s, args);
    return 0;
}
