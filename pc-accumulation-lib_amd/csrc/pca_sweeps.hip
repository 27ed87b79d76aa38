// pca_sweeps.hip -- K0s: the lidar sweeps of one NuScenes sample merged into the keyframe's lidar frame, every point
// labelled with the ground-truth box it lies in (include/pca.h: pca_nusc_merge_sweeps).
//
// The per-point part of the reference's inst_centric_get_sweeps (datasets/nuscenes_utils.py:233-243, :312-329, :332-531):
// the radius filter, the f64 transform stored back as f32, one point-in-box test per (point, candidate box of the point's
// sweep) and the instance / class columns.  The SPLIT form of the project's stable compaction:
//   swp_front   one workgroup per tile of 512 points of ONE sweep: filter, transform, box loop (the box table comes through
//               scalar loads: it is uniform across the workgroup), per-box hit counts in LDS -> at most one global atomic
//               per (workgroup, box with a hit), the kept points and the index of their last containing box into the
//               tile's own staging rows, the tile's count;
//   swp_append  adds up the counts of the tiles before its own (as k1n_append_batch does), rebuilds the box -> track table
//               in LDS from the hit counts swp_front left (same stream: no waiting on other workgroups anywhere) and writes
//               the finished rows.
// The host tables reach the device through the context's pinned block, fetched by a kernel that also clears the hit counts.
#include <cmath>
#include "pca_common.h"

#define SWP_BLK 256
#define SWP_PPT 2
#define SWP_TILE (SWP_BLK * SWP_PPT)
#define SWP_NW (SWP_BLK / PCA_WAVE)
static_assert(SWP_TILE == 512, "pca.h promises tiles of 512 points");

struct SwpSweep {              // device form of pca_nusc_sweep
    double T[12];
    int32_t row0, n, box0, nbox, tile0, ntiles;
    float lag, sweep;
};
struct SwpBox {                // device form of pca_nusc_sweep_box, with the certified bounds of the pre-test
    double inv[12];
    double size[3];
    double lo[3];              // |local| below this: inside on that axis for certain (0: never certain)
    double hi[3];              // |local| above this: outside for certain (inf: never certain)
    int32_t cls, key;
};
static_assert(sizeof(SwpSweep) == 128 && sizeof(SwpBox) == 176, "table records are moved in 16-byte words");

struct SwpArgs {
    const float *raw;
    const SwpSweep *sweeps;
    const SwpBox *boxes;
    int32_t n_sweeps, n_boxes;
    float radius;
    double limit;
    uint32_t *counts;          // [tiles] kept points of the tile
    int32_t *last;             // [tiles] the sweep this tile is the last one of, or -1
    float4 *sxyzi;             // [tiles * SWP_TILE] staged x', y', z', intensity
    int32_t *sbox;             // [tiles * SWP_TILE] staged index of the last containing box, or -1
    float *out;                // [<= n][8]
    int32_t *sweep_off;        // [n_sweeps + 1]
    uint32_t *hits;            // [n_boxes]
};

__global__ __launch_bounds__(256) void swp_fetch(const uint4 *src, uint4 *dst, int64_t n16, uint32_t *hits, int n_hits)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += stride) dst[i] = src[i];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_hits; i += stride) hits[i] = 0u;
}

// the sweep a tile belongs to (at most 32 sweeps: a scan of the table's tile0 column through scalar loads)
__device__ __forceinline__ int swp_sweep_of(const SwpArgs &a, int tile)
{
    int s = 0;
    for (int k = 1; k < a.n_sweeps; ++k)
        if (tile >= pca_sload(&a.sweeps[k].tile0)) s = k;
    return s;
}

__device__ __forceinline__ uint32_t swp_lanes_below(uint64_t m)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__global__ __launch_bounds__(SWP_BLK) void swp_front(const SwpArgs a)
{
    __shared__ uint32_t s_hits[PCA_NUSC_MAX_SWEEP_BOXES];
    __shared__ uint32_t s_cnt[SWP_PPT * SWP_NW];
    const int tile = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = swp_sweep_of(a, tile);
    const SwpSweep *sp = a.sweeps + s;
    const int tile0 = pca_sload(&sp->tile0), ntiles = pca_sload(&sp->ntiles);
    const int n = pca_sload(&sp->n), nbox = pca_sload(&sp->nbox), box0 = pca_sload(&sp->box0);
    const int64_t first = (int64_t)pca_sload(&sp->row0) + (int64_t)(tile - tile0) * SWP_TILE;
    const int left = n - (tile - tile0) * SWP_TILE;
    const int n_here = left < SWP_TILE ? (left < 0 ? 0 : left) : SWP_TILE;
    double T[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = pca_sload(&sp->T[i]);
    for (int b = threadIdx.x; b < nbox; b += SWP_BLK) s_hits[b] = 0u;

    bool keep[SWP_PPT];
    float xf[SWP_PPT], yf[SWP_PPT], zf[SWP_PPT], inten[SWP_PPT];
    int last[SWP_PPT];
#pragma unroll
    for (int k = 0; k < SWP_PPT; ++k) {
        const int p = k * SWP_BLK + (int)threadIdx.x;
        const bool valid = p < n_here;
        const float *row = a.raw + (first + p) * 5;
        const float x = valid ? pca_ldg(row) : 0.f, y = valid ? pca_ldg(row + 1) : 0.f, z = valid ? pca_ldg(row + 2) : 0.f;
        inten[k] = valid ? pca_ldg(row + 3) : 0.f;
        // np.linalg.norm of the f32 pair: every step a correctly rounded f32 operation; a NaN compares false
        keep[k] = valid && __fsqrt_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y))) > a.radius;
        xf[k] = (float)row4(T + 0, (double)x, (double)y, (double)z);
        yf[k] = (float)row4(T + 4, (double)x, (double)y, (double)z);
        zf[k] = (float)row4(T + 8, (double)x, (double)y, (double)z);
        last[k] = -1;
    }
    __syncthreads();
    const double L = a.limit;
    for (int b = 0; b < nbox; ++b) {
        const SwpBox *bx = a.boxes + box0 + b;
        double inv[12], size[3], lo[3], hi[3];
#pragma unroll
        for (int i = 0; i < 12; ++i) inv[i] = pca_sload(&bx->inv[i]);
#pragma unroll
        for (int i = 0; i < 3; ++i) { size[i] = pca_sload(&bx->size[i]); lo[i] = pca_sload(&bx->lo[i]); hi[i] = pca_sload(&bx->hi[i]); }
#pragma unroll
        for (int k = 0; k < SWP_PPT; ++k) {
            const double x = (double)xf[k], y = (double)yf[k], z = (double)zf[k];
            const double lx = row4(inv + 0, x, y, z), ly = row4(inv + 4, x, y, z), lz = row4(inv + 8, x, y, z);
            const double ax = fabs(lx), ay = fabs(ly), az = fabs(lz);
            bool in;
            // lo / hi bracket size * limit by more than the division's rounding can move the quotient across `limit`
            // (swp_bounds): between them -- and for a NaN, which fails both comparisons -- the division decides
            if (ax < lo[0] && ay < lo[1] && az < lo[2]) in = true;
            else if (ax > hi[0] || ay > hi[1] || az > hi[2]) in = false;
            else in = fabs(lx / size[0]) < L && fabs(ly / size[1]) < L && fabs(lz / size[2]) < L;
            in = in && keep[k];
            if (in) last[k] = b;
            const uint64_t m = __ballot(in);
            if (m != 0ull && lane == 0) atomicAdd(&s_hits[b], (uint32_t)__popcll(m));
        }
    }
    // stable ranks inside the tile (point order = k-major, then thread)
    uint32_t local[SWP_PPT];
#pragma unroll
    for (int k = 0; k < SWP_PPT; ++k) {
        const uint64_t m = __ballot(keep[k]);
        local[k] = swp_lanes_below(m);
        if (lane == 0) s_cnt[k * SWP_NW + wave] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < nbox; b += SWP_BLK) {
        const uint32_t c = s_hits[b];
        if (c) atomicAdd(a.hits + box0 + b, c);
    }
    uint32_t total = 0;
#pragma unroll
    for (int i = 0; i < SWP_PPT * SWP_NW; ++i) total += s_cnt[i];
    const int64_t sbase = (int64_t)tile * SWP_TILE;
#pragma unroll
    for (int k = 0; k < SWP_PPT; ++k) {
        if (!keep[k]) continue;
        uint32_t off = 0;
        for (int i = 0; i < k * SWP_NW + wave; ++i) off += s_cnt[i];
        const int64_t o = sbase + off + local[k];
        a.sxyzi[o] = make_float4(xf[k], yf[k], zf[k], inten[k]);
        a.sbox[o] = last[k] >= 0 ? box0 + last[k] : -1;
    }
    if (threadIdx.x == 0) {
        a.counts[tile] = total;
        a.last[tile] = tile - tile0 == ntiles - 1 ? s : -1;
    }
}

__global__ __launch_bounds__(256) void swp_append(const SwpArgs a)
{
    constexpr int BLK = 256, NW = BLK / 64;
    __shared__ uint32_t s_first[PCA_NUSC_MAX_SWEEP_BOXES];    // per track key: its first box with a hit
    __shared__ uint32_t s_trk[PCA_NUSC_MAX_SWEEP_BOXES];      // per track key: the track's index
    __shared__ uint32_t s_w[NW];
    const int tile = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t sum = 0;
    for (int t = threadIdx.x; t < tile; t += BLK) sum += pca_ldg(a.counts + t);
    sum = wave_reduce_add(sum);
    if (lane == 0) s_w[wave] = sum;
    const uint32_t c = pca_sload(a.counts + tile);
    const int32_t lf = pca_sload(a.last + tile);
    __syncthreads();
    uint32_t before = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) before += s_w[w];
    if (threadIdx.x == 0) {
        if (tile == 0) a.sweep_off[0] = 0;
        if (lf >= 0) a.sweep_off[lf + 1] = (int32_t)(before + c);
    }
    if (c == 0) return;                                       // (uniform: nothing of this tile was kept)
    // box -> track: box b opens a track iff it has a hit and no earlier box of its key has; tracks count up in box order
    const int nb = a.n_boxes;
    for (int b = threadIdx.x; b < nb; b += BLK) s_first[b] = 0xffffffffu;
    __syncthreads();
    for (int b = threadIdx.x; b < nb; b += BLK)
        if (pca_ldg(a.hits + b) > 0u) atomicMin(&s_first[pca_ldg(&a.boxes[b].key)], (uint32_t)b);
    __syncthreads();
    uint32_t opened = 0;
    for (int b0 = 0; b0 < nb; b0 += BLK) {
        const int b = b0 + (int)threadIdx.x;
        int key = 0;
        bool open = false;
        if (b < nb && pca_ldg(a.hits + b) > 0u) {
            key = pca_ldg(&a.boxes[b].key);
            open = s_first[key] == (uint32_t)b;
        }
        const uint64_t m = __ballot(open);
        if (lane == 0) s_w[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t off = opened, all = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) { if (w < wave) off += s_w[w]; all += s_w[w]; }
        if (open) s_trk[key] = off + swp_lanes_below(m);
        opened += all;
        __syncthreads();
    }
    const int s = swp_sweep_of(a, tile);
    const float lag = pca_sload(&a.sweeps[s].lag), sweep = pca_sload(&a.sweeps[s].sweep);
    const int64_t sbase = (int64_t)tile * SWP_TILE;
    for (uint32_t j = threadIdx.x; j < c; j += BLK) {
        const float4 v = a.sxyzi[sbase + j];
        const int32_t lb = pca_ldg(a.sbox + sbase + j);
        float inst = -1.f, cls = -1.f;
        if (lb >= 0) {
            inst = (float)s_trk[pca_ldg(&a.boxes[lb].key)];
            cls = (float)pca_ldg(&a.boxes[lb].cls);
        }
        float4 *o = reinterpret_cast<float4 *>(a.out + ((int64_t)before + j) * 8);
        o[0] = v;
        o[1] = make_float4(lag, sweep, inst, cls);
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// The workspace, byte offsets (every region on a 256-byte boundary).  The first two regions are the block that travels from
// the pinned block before the launch; `tiles` bounds the tiles of any split of n_points rows into at most 32 sweeps.
struct SwpWsLayout { int64_t sweeps, boxes, counts, last, sxyzi, sbox, tables_bytes, total; };
static SwpWsLayout swp_ws_layout(int64_t n_points, int n_boxes)
{
    const int64_t tiles = n_points / SWP_TILE + PCA_NUSC_MAX_SWEEPS + 1;
    SwpWsLayout l;
    l.sweeps = 0;
    l.boxes = l.sweeps + pca_align256((int64_t)sizeof(SwpSweep) * PCA_NUSC_MAX_SWEEPS);
    l.tables_bytes = l.boxes + pca_align256((int64_t)sizeof(SwpBox) * n_boxes);
    l.counts = l.tables_bytes;
    l.last = l.counts + pca_align256(tiles * 4);
    l.sxyzi = l.last + pca_align256(tiles * 4);
    l.sbox = l.sxyzi + tiles * SWP_TILE * 16;
    l.total = l.sbox + tiles * SWP_TILE * 4 + 256;
    return l;
}

extern "C" int64_t pca_nusc_merge_sweeps_workspace_bytes(int64_t n_points, int n_boxes)
{
    if (n_points < 0 || n_boxes < 0) return -1;
    return swp_ws_layout(n_points, n_boxes).total;
}

// |local| < lo  =>  fabs(local / size) < limit, and |local| > hi  =>  not, for every rounding of the division:
// t = fl(|size| * limit) is within 2^-53 (relative) of the product, fl(t * (1 -+ 2^-50)) within another 2^-53, so lo lies
// below and hi above |size| * limit by a factor of more than 1 -+ 2^-51; a quotient that far from `limit` is at least two
// units in the last place away from it and cannot be rounded onto or across it.  Outside the range where those relative
// bounds hold (tiny, huge, zero, non-finite) the pre-test never answers: lo = 0, hi = inf.
static void swp_bounds(double size, double limit, bool on, double *lo, double *hi)
{
    const double s = fabs(size);
    *lo = 0.0; *hi = INFINITY;
    if (on && limit > 0x1p-500 && limit < 0x1p500 && s > 0x1p-500 && s < 0x1p500) {
        const double t = s * limit;
        *lo = t * (1.0 - 0x1p-50);
        *hi = t * (1.0 + 0x1p-50);
    }
}

extern "C" int pca_nusc_merge_sweeps(pca_ctx *ctx, const float *raw, int64_t n_points, const pca_nusc_sweep *sweeps,
                                     int n_sweeps, const pca_nusc_sweep_box *boxes, int n_boxes, float center_radius,
                                     double inside_limit, void *workspace, int64_t workspace_bytes, float *points_out,
                                     int32_t *tally_out, void *stream)
{
    if (!ctx) return -1;
    if (n_sweeps > PCA_NUSC_MAX_SWEEPS) { ctx->err = "nusc sweeps: at most " + std::to_string(PCA_NUSC_MAX_SWEEPS) + " sweeps per call"; return -1; }
    if (n_boxes > PCA_NUSC_MAX_SWEEP_BOXES) { ctx->err = "nusc sweeps: at most " + std::to_string(PCA_NUSC_MAX_SWEEP_BOXES) + " boxes per call"; return -1; }
    if (n_sweeps < 1 || n_boxes < 0 || n_points < 0 || !sweeps || (n_boxes > 0 && !boxes) || (n_points > 0 && (!raw || !points_out)) ||
        !workspace || !tally_out) { ctx->err = "nusc sweeps: bad arguments"; return -1; }
    int64_t tiles = 0, rows = 0;
    for (int k = 0; k < n_sweeps; ++k) {
        const pca_nusc_sweep &sw = sweeps[k];
        if (sw.row0 < 0 || sw.n_rows < 0 || (int64_t)sw.row0 + sw.n_rows > n_points || sw.box0 < 0 || sw.n_boxes < 0 ||
            (int64_t)sw.box0 + sw.n_boxes > n_boxes) { ctx->err = "nusc sweeps: a sweep's rows or boxes lie outside the tables"; return -1; }
        rows += sw.n_rows;
        tiles += sw.n_rows > 0 ? ((int64_t)sw.n_rows + SWP_TILE - 1) / SWP_TILE : 1;
    }
    if (tiles > PCA_NUSC_MAX_SWEEP_TILES) {
        ctx->err = "nusc sweeps: at most " + std::to_string(PCA_NUSC_MAX_SWEEP_TILES) + " tiles of " + std::to_string(SWP_TILE) + " points per call";
        return -1;
    }
    for (int b = 0; b < n_boxes; ++b)
        if (boxes[b].track_key < 0 || boxes[b].track_key >= n_boxes) { ctx->err = "nusc sweeps: track_key must be in 0 .. n_boxes - 1"; return -1; }
    const SwpWsLayout l = swp_ws_layout(n_points, n_boxes);
    if (rows > n_points || tiles > n_points / SWP_TILE + PCA_NUSC_MAX_SWEEPS + 1) { ctx->err = "nusc sweeps: the sweeps' rows overlap"; return -1; }
    if (workspace_bytes < l.total) { ctx->err = "nusc sweeps: workspace too small"; return -1; }
    hipStream_t s = (hipStream_t)stream;
    PCA_CHECK(ctx, hipSetDevice(ctx->device));
    // the tables, built in the context's pinned block (free again once the fetch of the call before has run)
    if (ctx->k1n_busy) { PCA_CHECK(ctx, hipEventSynchronize(ctx->k1n_ev)); ctx->k1n_busy = false; }
    if (l.tables_bytes > ctx->k1n_pin_cap) {
        if (ctx->k1n_pin) PCA_CHECK(ctx, hipHostFree(ctx->k1n_pin));
        ctx->k1n_pin = nullptr; ctx->k1n_pin_cap = 0;
        PCA_CHECK(ctx, hipHostMalloc(&ctx->k1n_pin, (size_t)(2 * l.tables_bytes), hipHostMallocMapped));
        ctx->k1n_pin_cap = 2 * l.tables_bytes;
    }
    if (!ctx->k1n_ev) PCA_CHECK(ctx, hipEventCreateWithFlags(&ctx->k1n_ev, hipEventDisableTiming));
    char *pin = reinterpret_cast<char *>(ctx->k1n_pin);
    SwpSweep *hs = reinterpret_cast<SwpSweep *>(pin + l.sweeps);
    SwpBox *hb = reinterpret_cast<SwpBox *>(pin + l.boxes);
    int32_t tile0 = 0;
    for (int k = 0; k < n_sweeps; ++k) {
        const pca_nusc_sweep &sw = sweeps[k];
        for (int i = 0; i < 12; ++i) hs[k].T[i] = sw.T[i];
        hs[k].row0 = sw.row0; hs[k].n = sw.n_rows; hs[k].box0 = sw.box0; hs[k].nbox = sw.n_boxes;
        hs[k].tile0 = tile0; hs[k].ntiles = sw.n_rows > 0 ? (sw.n_rows + SWP_TILE - 1) / SWP_TILE : 1;
        hs[k].lag = sw.lag; hs[k].sweep = sw.sweep;
        tile0 += hs[k].ntiles;
    }
    const bool pretest = pca_env_int("PCA_NUSC_SWEEPS_PRETEST", 1) != 0;
    for (int b = 0; b < n_boxes; ++b) {
        for (int i = 0; i < 12; ++i) hb[b].inv[i] = boxes[b].inv[i];
        for (int i = 0; i < 3; ++i) {
            hb[b].size[i] = boxes[b].size[i];
            swp_bounds(boxes[b].size[i], inside_limit, pretest, &hb[b].lo[i], &hb[b].hi[i]);
        }
        hb[b].cls = boxes[b].cls; hb[b].key = boxes[b].track_key;
    }
    char *w = reinterpret_cast<char *>(workspace);
    SwpArgs a;
    a.raw = raw;
    a.sweeps = reinterpret_cast<const SwpSweep *>(w + l.sweeps);
    a.boxes = reinterpret_cast<const SwpBox *>(w + l.boxes);
    a.n_sweeps = n_sweeps; a.n_boxes = n_boxes; a.radius = center_radius; a.limit = inside_limit;
    a.counts = reinterpret_cast<uint32_t *>(w + l.counts); a.last = reinterpret_cast<int32_t *>(w + l.last);
    a.sxyzi = reinterpret_cast<float4 *>(w + l.sxyzi); a.sbox = reinterpret_cast<int32_t *>(w + l.sbox);
    a.out = points_out; a.sweep_off = tally_out; a.hits = reinterpret_cast<uint32_t *>(tally_out + n_sweeps + 1);
    void *src = nullptr;
    PCA_CHECK(ctx, hipHostGetDevicePointer(&src, ctx->k1n_pin, 0));
    const int64_t n16 = l.tables_bytes / 16;
    const int grid = (int)((n16 + 255) / 256 < 64 ? (n16 + 255) / 256 : 64);
    hipLaunchKernelGGL(swp_fetch, dim3(grid), dim3(256), 0, s, reinterpret_cast<const uint4 *>(src), reinterpret_cast<uint4 *>(w),
                       n16, a.hits, n_boxes);
    PCA_CHECK(ctx, hipEventRecord(ctx->k1n_ev, s));
    ctx->k1n_busy = true;
    hipLaunchKernelGGL(swp_front, dim3((unsigned)tiles), dim3(SWP_BLK), 0, s, a);
    hipLaunchKernelGGL(swp_append, dim3((unsigned)tiles), dim3(256), 0, s, a);
    PCA_CHECK(ctx, hipGetLastError());
    return 0;
}
