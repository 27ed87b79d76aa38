// pca_voxel_distance.hip -- how FAR every voxel of a label volume is from the nearest labelled one: the exact feature transform
// (squared distance, nearest site, its label) under an integer metric D = w_xy (drow^2 + dcol^2) + w_z dk^2, and the two things
// made of it in the same call: `filled` (an empty voxel takes the label of its nearest site within a radius) and `tsdf` (SSCNet's
// truncated, optionally flipped, signed distance).  The call reads volumes: no store, no points.
//
// The nearest site is the one that minimises the pair (D, q), q = (k' px + row') px + col' its linear place.  The rule separates by
// axis -- within one line all candidates share the other two offsets -- so each pass keeps its own lexicographic minimum of
// (partial D, q) and the result does not depend on the order of the passes.  Two launches, no atomics, no wait between workgroups:
//
//   voxel_dist_lines   the k pass and the col pass.  A workgroup takes a row of the volume and a round of its k values (all col; a
//                      grid-stride loop over rows x rounds; a round is a quarter of the k values, at most DIST_ITEMS places).
//                      1: a thread per col folds the column's label bytes into ONE word, bit k' = "(k', row, col) is a site"
//                      (the loads run along col; every round of a row builds the words again, from L2).  2: for the round's
//                      places (k, col) the k pass is bit arithmetic on that word -- the nearest set bit at or below k and the
//                      nearest above it; at equal distance the lower k' is the smaller place -- and leaves (g, q) in LDS.  3: the
//                      col pass of those lines, see dist_scan; the result goes to the workspace, along col.
//   voxel_dist_rows    the row pass and every output.  A workgroup takes, for one k, all rows of `tc` neighbouring columns (tc px
//                      <= DIST_ITEMS, tc <= 64: a tile is at most 48 KB of LDS), loads their (g, q) from the workspace -- runs of tc
//                      places, the strided axis -- scans along row with stride tc (neighbouring lanes, neighbouring columns: no
//                      bank conflict), and writes dist2 / nearest / nearest_label / filled / tsdf.  nearest_label is labels[q].
//
//   dist_scan          the exact minimum over one line of `n` candidates g(x') + w (x - x')^2 for the place x: the candidates are
//                      visited outwards, x, x -+ 1, x -+ 2, ..., and the walk ends as soon as w d^2 alone is MORE than the best
//                      found so far (g >= 0: nothing further out can win or tie) or than max_dist2, or when both ends of the line
//                      are passed.  A line without a finite g is not walked at all (a flag per line).  With sites every few voxels
//                      the walk is a few steps; with one site in the volume it is the whole line for every voxel, which is the
//                      worst case: 1024 steps of two LDS reads.  Every candidate is the true D of a real site, so it fits the
//                      int32 the limits promise (w_xy 2 (px-1)^2 + w_z (nz-1)^2 <= 2^31 - 2), and w d^2 <= 2^30; the compares
//                      are unsigned 32-bit with 0xffffffff = no site.
// Out of scope: distances in float metres for irrational cell ratios; grids above 1024; a .tsdf file; distance to free-space
// boundaries; how the fine volumes are made.
#include "pca_common.h"

#define DIST_THREADS 256
#define DIST_ITEMS 6144           // places (one u32 g and one i32 q each) a workgroup holds in LDS
#define DIST_MAX_TC 64
#define DIST_MAX_G 2048
#define DIST_NONE 0xffffffffu

struct alignas(16) DistArgs {
    int px, nz, G;
    int kc, rounds, line_tasks;   // lines: k values of a round (kc px <= DIST_ITEMS), rounds of a row, rows x rounds
    int tc, tiles_c, tiles;       // rows: columns of a tile, tiles per k, tiles in all
    uint32_t site_mask;           // bit l: label l makes a site
    uint32_t w_xy, w_z, lim;      // lim: min(max_dist2, 2^31 - 1)
    int fill_free, tsdf_flip;
    uint32_t fill_lim;
    double tsdf_unit, tsdf_trunc;
    const uint8_t *labels, *seen;
    uint32_t *ws_d;
    int32_t *ws_q;
    int32_t *dist2, *nearest;
    uint8_t *nearest_label, *filled;
    float *tsdf;
};

// the lexicographic minimum of (g[x' stride] + w (x - x')^2, q[x' stride]) over x' in 0 .. n-1, candidates above lim left out
__device__ __forceinline__ void dist_scan(const uint32_t *g, const int32_t *q, int stride, int n, int x, uint32_t w, uint32_t lim,
                                          uint32_t &best_d, int32_t &best_q)
{
    best_d = DIST_NONE; best_q = -1;
    {
        const uint32_t c = g[x * stride];
        if (c <= lim) { best_d = c; best_q = q[x * stride]; }     // (DIST_NONE > lim)
    }
    for (int d = 1; d < n; ++d) {
        const uint32_t wd = w * (uint32_t)(d * d);                // <= 2^30 (limits)
        if (wd > (best_d < lim ? best_d : lim)) break;
        const int lo = x - d, hi = x + d;
        if (lo < 0 && hi >= n) break;
        if (lo >= 0) {
            const uint32_t gl = g[lo * stride];
            if (gl != DIST_NONE) {
                const uint32_t c = gl + wd;                       // gl, c <= 2^31 - 2: the D of a real site
                if (c <= lim) {
                    const int32_t cq = q[lo * stride];
                    if (c < best_d || (c == best_d && cq < best_q)) { best_d = c; best_q = cq; }
                }
            }
        }
        if (hi < n) {
            const uint32_t gh = g[hi * stride];
            if (gh != DIST_NONE) {
                const uint32_t c = gh + wd;
                if (c <= lim) {
                    const int32_t cq = q[hi * stride];
                    if (c < best_d || (c == best_d && cq < best_q)) { best_d = c; best_q = cq; }
                }
            }
        }
    }
}

__global__ __launch_bounds__(DIST_THREADS) void voxel_dist_lines(const DistArgs a)
{
    __shared__ uint32_t s_g[DIST_ITEMS];
    __shared__ int32_t s_q[DIST_ITEMS];
    __shared__ uint32_t s_bits[1024];
    __shared__ int s_any;
    const int tid = (int)threadIdx.x, px = a.px, nz = a.nz;
    const int64_t plane = (int64_t)px * px;

    for (int task = (int)blockIdx.x; task < a.line_tasks; task += a.G) {
        const int row = task / a.rounds, k0 = (task - row * a.rounds) * a.kc;
        if (tid == 0) s_any = 0;
        __syncthreads();
        // 1: the sites of the row's columns, a bit per k
        bool any = false;
        for (int col = tid; col < px; col += DIST_THREADS) {
            uint32_t bits = 0;
            const uint8_t *p = a.labels + (int64_t)row * px + col;
            for (int k = 0; k < nz; ++k) {
                const uint32_t l = pca_ldg(p + k * plane);
                if (l < PCA_BEV_VOXEL_MAX_LABELS && ((a.site_mask >> l) & 1u)) bits |= 1u << k;
            }
            s_bits[col] = bits;
            any |= bits != 0;
        }
        if (any) s_any = 1;       // (every writer stores the same value)
        __syncthreads();
        const bool walk = s_any != 0;
        {
            const int items = (nz - k0 < a.kc ? nz - k0 : a.kc) * px;
            if (walk) {
                // 2: the k pass
                for (int it = tid; it < items; it += DIST_THREADS) {
                    const int kl = it / px, col = it - kl * px, k = k0 + kl;
                    const uint32_t bits = s_bits[col];
                    const uint32_t below = bits & (0xffffffffu >> (31 - k)), above = k < 31 ? bits >> (k + 1) : 0u;
                    uint32_t g = DIST_NONE;
                    int ks = -1;
                    if (below) { ks = 31 - __clz((int)below); g = a.w_z * (uint32_t)((k - ks) * (k - ks)); }
                    if (above) {
                        const int ku = k + 1 + (__ffs((int)above) - 1);
                        const uint32_t gu = a.w_z * (uint32_t)((ku - k) * (ku - k));
                        if (gu < g) { g = gu; ks = ku; }          // (equal: the lower k' is the smaller place)
                    }
                    if (g > a.lim) g = DIST_NONE;
                    s_g[it] = g;
                    s_q[it] = g == DIST_NONE ? -1 : (int32_t)(((int64_t)ks * px + row) * px + col);
                }
                __syncthreads();
            }
            // 3: the col pass, out along col
            for (int it = tid; it < items; it += DIST_THREADS) {
                const int kl = it / px, col = it - kl * px;
                uint32_t bd = DIST_NONE;
                int32_t bq = -1;
                if (walk) dist_scan(s_g + kl * px, s_q + kl * px, 1, px, col, a.w_xy, a.lim, bd, bq);
                const int64_t at = ((int64_t)(k0 + kl) * px + row) * px + col;
                a.ws_d[at] = bd;
                a.ws_q[at] = bq;
            }
            __syncthreads();      // (the next task overwrites what this one's walkers read)
        }
    }
}

__global__ __launch_bounds__(DIST_THREADS) void voxel_dist_rows(const DistArgs a)
{
    __shared__ uint32_t s_g[DIST_ITEMS];
    __shared__ int32_t s_q[DIST_ITEMS];
    __shared__ int s_any[DIST_MAX_TC];
    const int tid = (int)threadIdx.x, px = a.px, tc = a.tc;

    for (int tile = (int)blockIdx.x; tile < a.tiles; tile += a.G) {
        const int k = tile / a.tiles_c, c0 = (tile - k * a.tiles_c) * tc;
        const int cols = px - c0 < tc ? px - c0 : tc, items = cols * px;      // items <= tc px <= DIST_ITEMS
        if (tid < DIST_MAX_TC) s_any[tid] = 0;
        __syncthreads();
        for (int it = tid; it < items; it += DIST_THREADS) {
            const int row = it / cols, c = it - row * cols;
            const int64_t at = ((int64_t)k * px + row) * px + c0 + c;
            const uint32_t g = pca_ldg(a.ws_d + at);
            s_g[it] = g;
            s_q[it] = pca_ldg(a.ws_q + at);
            if (g != DIST_NONE) s_any[c] = 1;                                 // (every writer stores the same value)
        }
        __syncthreads();
        for (int it = tid; it < items; it += DIST_THREADS) {
            const int row = it / cols, c = it - row * cols;
            const int64_t at = ((int64_t)k * px + row) * px + c0 + c;
            uint32_t bd = DIST_NONE;
            int32_t bq = -1;
            if (s_any[c]) dist_scan(s_g + c, s_q + c, cols, px, row, a.w_xy, a.lim, bd, bq);
            const bool has = bd != DIST_NONE;
            if (a.dist2) a.dist2[at] = has ? (int32_t)bd : -1;
            if (a.nearest) a.nearest[at] = bq;
            uint32_t nl = 255u;
            if (has && (a.nearest_label || a.filled)) nl = pca_ldg(a.labels + bq);
            if (a.nearest_label) a.nearest_label[at] = (uint8_t)nl;
            if (a.filled || a.tsdf) {
                const uint32_t own = pca_ldg(a.labels + at);
                const bool empty = own >= PCA_BEV_VOXEL_MAX_LABELS;
                const bool unseen = !a.seen || pca_ldg(a.seen + at) == 0;     // (without `seen`: eligible, and never negative)
                if (a.filled) {
                    uint32_t f = 255u;
                    if (!empty) f = own;
                    else if (has && bd <= a.fill_lim && (a.fill_free || unseen)) f = nl;
                    a.filled[at] = (uint8_t)f;
                }
                if (a.tsdf) {
                    const double m = has ? fmin(sqrt((double)bd) * a.tsdf_unit, a.tsdf_trunc) / a.tsdf_trunc : 1.0;
                    const double v = a.tsdf_flip ? 1.0 - m : m;
                    const double sign = (a.seen && empty && unseen) ? -1.0 : 1.0;
                    a.tsdf[at] = (float)(sign * v);
                }
            }
        }
        __syncthreads();          // (the next tile overwrites what this one's walkers read)
    }
}

static int64_t dist_cells(int px, int nz) { return (int64_t)nz * px * px; }

extern "C" {

int64_t pca_voxel_distance_workspace_bytes(int px, int nz)
{
    if (px < 1 || px > 1024 || nz < 1 || nz > 32) return -1;
    return 2 * pca_align256(dist_cells(px, nz) * 4);
}

int pca_voxel_distance(pca_ctx *ctx, int px, int nz, const uint8_t *labels, const uint8_t *seen, const pca_class_group *site_labels,
                       int w_xy, int w_z, int64_t max_dist2, int64_t fill_dist2, int fill_free, double tsdf_unit, double tsdf_trunc,
                       int tsdf_flip, void *workspace, int64_t workspace_bytes, int32_t *dist2, int32_t *nearest,
                       uint8_t *nearest_label, uint8_t *filled, float *tsdf, void *stream)
{
    if (!ctx) return -1;
    hipStream_t s = (hipStream_t)stream;
    const std::string w("voxel distance");
    // every check comes before the first launch
    if (px < 1 || px > 1024) { ctx->err = w + ": px must be in 1..1024"; return -1; }
    if (nz < 1 || nz > 32) { ctx->err = w + ": nz must be in 1..32"; return -1; }
    if (w_xy < 1 || w_z < 1) { ctx->err = w + ": w_xy and w_z must be >= 1"; return -1; }
    {
        // (each product below 2^63: w < 2^31, 2 (px-1)^2 < 2^22, (nz-1)^2 < 2^10)
        const int64_t far = (int64_t)w_xy * 2 * (px - 1) * (px - 1) + (int64_t)w_z * (nz - 1) * (nz - 1);
        if (far > 2147483646ll) { ctx->err = w + ": w_xy 2 (px-1)^2 + w_z (nz-1)^2 must not exceed 2^31 - 2"; return -1; }
    }
    if (!labels) { ctx->err = w + ": labels must not be NULL"; return -1; }
    if (!dist2 && !nearest && !nearest_label && !filled && !tsdf) { ctx->err = w + ": at least one output is needed"; return -1; }
    if (tsdf && !(std::isfinite(tsdf_unit) && tsdf_unit > 0 && std::isfinite(tsdf_trunc) && tsdf_trunc > 0)) {
        ctx->err = w + ": tsdf needs tsdf_unit and tsdf_trunc finite and > 0"; return -1;
    }
    if (filled && fill_dist2 < 0) { ctx->err = w + ": filled needs fill_dist2 >= 0"; return -1; }
    const int64_t cells = dist_cells(px, nz), need = pca_voxel_distance_workspace_bytes(px, nz);
    if (!workspace || workspace_bytes < need) { ctx->err = w + ": workspace too small (pca_voxel_distance_workspace_bytes)"; return -1; }
    if ((uintptr_t)workspace & 3) { ctx->err = w + ": workspace must be 4-byte aligned"; return -1; }

    DistArgs A;
    A.px = px; A.nz = nz;
    A.site_mask = site_labels ? (uint32_t)site_labels->mask[0] : 0xffffffffu;       // labels are below 32
    A.w_xy = (uint32_t)w_xy; A.w_z = (uint32_t)w_z;
    A.lim = (max_dist2 < 0 || max_dist2 > 2147483647ll) ? 2147483647u : (uint32_t)max_dist2;
    A.fill_free = fill_free != 0; A.tsdf_flip = tsdf_flip != 0;
    A.fill_lim = (fill_dist2 < 0) ? 0u : (fill_dist2 > 2147483647ll ? 2147483647u : (uint32_t)fill_dist2);
    A.tsdf_unit = tsdf_unit; A.tsdf_trunc = tsdf_trunc;
    A.labels = labels; A.seen = seen;
    A.ws_d = reinterpret_cast<uint32_t *>(workspace);
    A.ws_q = reinterpret_cast<int32_t *>(reinterpret_cast<uint8_t *>(workspace) + pca_align256(cells * 4));
    A.dist2 = dist2; A.nearest = nearest; A.nearest_label = nearest_label; A.filled = filled; A.tsdf = tsdf;
    // a row's k values in at least four rounds where there are that many: a row alone is too few workgroups for the device at 256
    A.kc = (nz + 3) / 4 < DIST_ITEMS / px ? (nz + 3) / 4 : DIST_ITEMS / px;          // 1 .. 8
    A.rounds = (nz + A.kc - 1) / A.kc;
    A.line_tasks = px * A.rounds;                                                    // at most 1024 * 6
    A.tc = DIST_ITEMS / px < DIST_MAX_TC ? DIST_ITEMS / px : DIST_MAX_TC;           // >= 6
    if (A.tc > px) A.tc = px;
    A.tiles_c = (px + A.tc - 1) / A.tc;
    A.tiles = A.tiles_c * nz;                                                        // at most 171 * 32
    // PCA_VOXEL_DIST_G: a cap on the workgroups of both kernels, read on every call (tests send a workgroup round its loop again)
    const int max_g = (int)pca_env_int("PCA_VOXEL_DIST_G", DIST_MAX_G, 1, DIST_MAX_G);
    PCA_CHECK(ctx, hipSetDevice(ctx->device));
    A.G = A.line_tasks < max_g ? A.line_tasks : max_g;
    {
        const DistArgs &args = A;
        PCA_LAUNCH(ctx, PCA_K_VOXEL_DIST_LINES, voxel_dist_lines, dim3(args.G), dim3(DIST_THREADS), s, args);
    }
    A.G = A.tiles < max_g ? A.tiles : max_g;
    {
        const DistArgs &args = A;
        PCA_LAUNCH(ctx, PCA_K_VOXEL_DIST_ROWS, voxel_dist_rows, dim3(args.G), dim3(DIST_THREADS), s, args);
    }
    PCA_CHECK(ctx, hipGetLastError());
    return 0;
}

}  // extern "C"
