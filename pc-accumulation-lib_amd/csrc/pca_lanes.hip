// pca_lanes.hip -- KL: the ground-truth lane centrelines of a whole map clipped to the BEV of S samples at once
// (include/pca.h: pca_lanes_transform, pca_lanes_to_grid).
//
// The per-lane loop of the reference's generate() (bev_generator.py:101-109: preprocess_pc_and_trajs on a dummy cloud with
// every lane of the city map, then "remove empty lanes"; geometric_transform(is_traj=True) :207-237, crop_trajectory /
// cal_intersec_pnt :257-371 and pos2grid :737-747 underneath) as data-parallel work: ONE thread per edge (a -> b) of the
// packed vertex array, with the arithmetic of pca_host_ego_to_grid (pca_api.hip), step for step.
//   lanes_count  one workgroup per (tile of 256 edges, sample): both ends rotated and classified, 0 / 1 / 2 rows per edge,
//                the tile's total;
//   lanes_scan   one workgroup per sample: exclusive scan of the tile totals, the sample's row count;
//   lanes_emit   recomputes, ranks the edges inside the tile with two ballots and writes the rows -- edge order, which is
//                map order; no atomics decide a position.  Only a crossing edge runs the bisection.
// An edge exists where two consecutive vertices carry the same lane index: the pair (last vertex of lane i, first vertex of
// lane i + 1) is never one.
#include <cmath>
#include "pca_common.h"

#define LN_BLK 256
#define LN_NW (LN_BLK / PCA_WAVE)
// Halving an f64 gap from the largest finite value down to 1e-4 takes fewer than 1100 steps; a gap that is not a number
// ends the loop at once (the comparison fails), as it does in the reference.
#define LN_MAX_BISECT 1100

struct LnView {                // device form of pca_lane_view (16 doubles)
    double origin[3];
    double R[9];
    double dx, dy, view, px;
};
static_assert(sizeof(LnView) == 128 && sizeof(pca_lane_view) == 128, "views are moved in 16-byte words");

struct LnArgs {
    const double *xyz;         // [P][3]
    const int32_t *vlane;      // [P]
    int64_t n_edges;           // P - 1
    int32_t tiles;             // ceil(n_edges / 256)
    const LnView *views;       // [S]
    uint32_t *tile_rows;       // [S][tiles]: the tile's rows (lanes_count), then the rows before the tile (lanes_scan)
    int64_t cap;
    double *rows;              // [S][cap][3]
    int32_t *row_lane;         // [S][cap]
    int64_t *n_rows;           // [S]
    uint32_t *status;
};

struct LnFrame {               // one sample's view in registers (scalar loads: uniform across the workgroup)
    double o[3], R[9], dx, dy, view, px, h;
};

__device__ __forceinline__ LnFrame ln_frame(const LnView *v)
{
    LnFrame f;
#pragma unroll
    for (int i = 0; i < 3; ++i) f.o[i] = pca_sload(&v->origin[i]);
#pragma unroll
    for (int i = 0; i < 9; ++i) f.R[i] = pca_sload(&v->R[i]);
    f.dx = pca_sload(&v->dx); f.dy = pca_sload(&v->dy); f.view = pca_sload(&v->view); f.px = pca_sload(&v->px);
    f.h = 0.5 * f.view;
    return f;
}

// A NaN that no operand brought along is the invalid operation's own (0 * inf, inf - inf: a vertex that is not finite meets
// the zeros of a planar matrix).  IEEE 754 leaves its sign open: gfx950 clears it, the x86-64 hosts that run the reference's
// numpy and pca_host_ego_to_grid set it -- and the rows are held to the host's bit for bit.
__device__ __forceinline__ double ln_host_nan(double v, bool nan_in)
{
    return (v != v && !nan_in) ? __longlong_as_double((long long)0xfff8000000000000ull) : v;
}

// p - origin, then the rot lambda of pca_host_ego_to_grid: numpy's product adds onto +0.0, term by term in k order, so a
// stored z of -0.0 comes out +0.0 even where every product is a -0.0
__device__ __forceinline__ void ln_vertex(const LnFrame &f, const double *p, double &x, double &y, double &z)
{
    const double px = pca_ldg(p) - f.o[0], py = pca_ldg(p + 1) - f.o[1], pz = pca_ldg(p + 2) - f.o[2];
    const bool nan_in = px != px || py != py || pz != pz;
    x = ln_host_nan(fma(f.R[2], pz, fma(f.R[1], py, fma(f.R[0], px, 0.0))) + f.dx, nan_in);
    y = ln_host_nan(fma(f.R[5], pz, fma(f.R[4], py, fma(f.R[3], px, 0.0))) + f.dy, nan_in);
    z = ln_host_nan(fma(f.R[8], pz, fma(f.R[7], py, fma(f.R[6], px, 0.0))), nan_in);
}

__device__ __forceinline__ bool ln_inside(double x, double y, double h) { return -h < x && x < h && -h < y && y < h; }

struct LnEdge { double ax, ay, az, bx, by; bool a_in, cross; };

__device__ __forceinline__ LnEdge ln_edge(const LnArgs &a, const LnFrame &f, int64_t e)
{
    LnEdge g;
    g.a_in = false; g.cross = false;
    g.ax = g.ay = g.az = g.bx = g.by = 0.0;
    if (e < a.n_edges && pca_ldg(a.vlane + e) == pca_ldg(a.vlane + e + 1)) {
        double bz;
        ln_vertex(f, a.xyz + 3 * e, g.ax, g.ay, g.az);
        ln_vertex(f, a.xyz + 3 * (e + 1), g.bx, g.by, bz);
        g.a_in = ln_inside(g.ax, g.ay, f.h);
        g.cross = g.a_in != ln_inside(g.bx, g.by, f.h);
    }
    return g;
}

__global__ __launch_bounds__(LN_BLK) void lanes_count(const LnArgs a)
{
    __shared__ uint32_t s_w[LN_NW];
    const int tile = blockIdx.x, s = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const LnFrame f = ln_frame(a.views + s);
    const LnEdge g = ln_edge(a, f, (int64_t)tile * LN_BLK + threadIdx.x);
    const uint32_t c = (uint32_t)__popcll(__ballot(g.a_in)) + (uint32_t)__popcll(__ballot(g.cross));
    if (lane == 0) s_w[wave] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < LN_NW; ++w) t += s_w[w];
        a.tile_rows[(int64_t)s * a.tiles + tile] = t;
    }
}

__global__ __launch_bounds__(LN_BLK) void lanes_scan(const LnArgs a)
{
    __shared__ uint32_t s_w[LN_NW];
    const int s = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t *t = a.tile_rows + (int64_t)s * a.tiles;
    uint64_t before = 0;                                      // rows of the chunks already done (uniform)
    for (int t0 = 0; t0 < a.tiles; t0 += LN_BLK) {
        const int i = t0 + (int)threadIdx.x;
        const uint32_t c = i < a.tiles ? t[i] : 0u;
        const uint32_t incl = wave_incl_scan_add(c);
        if (lane == 63) s_w[wave] = incl;
        __syncthreads();
        uint32_t off = 0, all = 0;
#pragma unroll
        for (int w = 0; w < LN_NW; ++w) { if (w < wave) off += s_w[w]; all += s_w[w]; }
        // (a sample has at most 2 (P - 1) < 2^32 rows: pca_lanes_to_grid refuses more vertices)
        if (i < a.tiles) t[i] = (uint32_t)before + off + incl - c;
        before += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) a.n_rows[s] = (int64_t)before;
}

__device__ __forceinline__ uint32_t ln_lanes_below(uint64_t m)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__device__ __forceinline__ void ln_store(const LnArgs &a, const LnFrame &f, int s, int64_t pos, double x, double y, double z, int32_t lane_idx)
{
    if (pos >= a.cap) return;                                 // the count stays true: the caller runs the sample again
    double *r = a.rows + ((int64_t)s * a.cap + pos) * 3;
    r[0] = floor(x / f.view * f.px + 0.5 * f.px);
    r[1] = floor(y / f.view * f.px + 0.5 * f.px);
    r[2] = z;
    a.row_lane[(int64_t)s * a.cap + pos] = lane_idx;
}

__global__ __launch_bounds__(LN_BLK) void lanes_emit(const LnArgs a)
{
    __shared__ uint32_t s_w[LN_NW];
    const int tile = blockIdx.x, s = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const LnFrame f = ln_frame(a.views + s);
    const int64_t e = (int64_t)tile * LN_BLK + threadIdx.x;
    const LnEdge g = ln_edge(a, f, e);
    const uint64_t m_in = __ballot(g.a_in), m_x = __ballot(g.cross);
    if (lane == 0) s_w[wave] = (uint32_t)__popcll(m_in) + (uint32_t)__popcll(m_x);
    __syncthreads();
    uint32_t off = pca_sload(a.tile_rows + (int64_t)s * a.tiles + tile);
    for (int w = 0; w < wave; ++w) off += s_w[w];
    if (!g.a_in && !g.cross) return;
    int64_t pos = (int64_t)off + ln_lanes_below(m_in) + ln_lanes_below(m_x);
    const int32_t li = pca_ldg(a.vlane + e);
    if (g.a_in) ln_store(a, f, s, pos++, g.ax, g.ay, g.az, li);
    if (g.cross) {
        // cal_intersec_pnt (bev_generator.py:317-371): the midpoint replaces whichever end lies on its own side
        const double h = f.h;
        double x0 = g.ax, y0 = g.ay, x1 = g.bx, y1 = g.by, xm = 0.0, ym = 0.0, gap = __builtin_huge_val();
        int it = 0;
        for (; it < LN_MAX_BISECT && gap > 1e-4; ++it) {
            xm = 0.5 * (x0 + x1);
            ym = 0.5 * (y0 + y1);
            const bool p0_in = ln_inside(x0, y0, h), mid_in = ln_inside(xm, ym, h);
            if (mid_in == p0_in) { gap = sqrt((xm - x0) * (xm - x0) + (ym - y0) * (ym - y0)); x0 = xm; y0 = ym; }
            else { gap = sqrt((xm - x1) * (xm - x1) + (ym - y1) * (ym - y1)); x1 = xm; y1 = ym; }
        }
        if (gap > 1e-4) pca_raise(a.status, PCA_STATUS_LANES_BISECT_CAP);
        ln_store(a, f, s, pos, xm, ym, g.az, li);
    }
}

// xyz <- (T [p; 1])[:3] in place: numpy's (4,4) @ (4,N) product, the f64 fma chain in k order of K1n / K2 (row4) -- begun
// from +0.0, as numpy begins it, which decides the sign of a zero result
__device__ __forceinline__ double ln_row4(const double *r, double x, double y, double z)
{
    return fma(r[3], 1.0, fma(r[2], z, fma(r[1], y, fma(r[0], x, 0.0))));
}
__global__ __launch_bounds__(LN_BLK) void lanes_transform(double *xyz, int64_t n, const double t0, const double t1, const double t2,
                                                          const double t3, const double t4, const double t5, const double t6,
                                                          const double t7, const double t8, const double t9, const double t10,
                                                          const double t11)
{
    const int64_t i = (int64_t)blockIdx.x * LN_BLK + threadIdx.x;
    if (i >= n) return;
    const double T[12] = {t0, t1, t2, t3, t4, t5, t6, t7, t8, t9, t10, t11};
    double *p = xyz + 3 * i;
    const double x = p[0], y = p[1], z = p[2];
    const bool nan_in = x != x || y != y || z != z;
    p[0] = ln_host_nan(ln_row4(T + 0, x, y, z), nan_in);
    p[1] = ln_host_nan(ln_row4(T + 4, x, y, z), nan_in);
    p[2] = ln_host_nan(ln_row4(T + 8, x, y, z), nan_in);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
#define LN_MAX_VERTICES (1ll << 30)
#define LN_MAX_SAMPLES 65535           // grid.y

struct LnWsLayout { int64_t views, tile_rows, total; int32_t tiles; };
static LnWsLayout ln_ws_layout(int64_t P, int S)
{
    LnWsLayout l;
    l.tiles = (int32_t)(P > 1 ? (P - 1 + LN_BLK - 1) / LN_BLK : 0);
    l.views = 0;
    l.tile_rows = pca_align256((int64_t)sizeof(LnView) * S);
    l.total = l.tile_rows + pca_align256((int64_t)S * l.tiles * 4) + 256;
    return l;
}

extern "C" int64_t pca_lanes_workspace_bytes(int64_t n_vertices, int n_samples, int64_t cap_rows)
{
    if (n_vertices < 0 || n_vertices > LN_MAX_VERTICES || n_samples < 0 || n_samples > LN_MAX_SAMPLES || cap_rows < 0) return -1;
    return ln_ws_layout(n_vertices, n_samples).total;
}

extern "C" int pca_lanes_transform(pca_ctx *ctx, double *xyz, int64_t P, const double T[16], void *stream)
{
    if (!ctx) return -1;
    if (P < 0 || P > LN_MAX_VERTICES || !T || (P > 0 && !xyz)) { ctx->err = "lanes transform: bad arguments"; return -1; }
    if (P == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    PCA_CHECK(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(lanes_transform, dim3((unsigned)((P + LN_BLK - 1) / LN_BLK)), dim3(LN_BLK), 0, s, xyz, P, T[0], T[1], T[2],
                       T[3], T[4], T[5], T[6], T[7], T[8], T[9], T[10], T[11]);
    PCA_CHECK(ctx, hipGetLastError());
    return 0;
}

extern "C" int pca_lanes_to_grid(pca_ctx *ctx, const double *xyz, const int32_t *vertex_lane, const int32_t *start, int64_t P,
                                 int32_t L, const pca_lane_view *views, int S, int64_t cap_rows, double *rows, int32_t *row_lane,
                                 int64_t *n_rows, void *ws, void *stream)
{
    if (!ctx) return -1;
    if (P < 0 || P > LN_MAX_VERTICES || L < 0 || S < 0 || S > LN_MAX_SAMPLES || cap_rows < 0 || (S > 0 && (!views || !n_rows)) ||
        (P > 0 && L > 0 && (!xyz || !vertex_lane || !start)) || (cap_rows > 0 && S > 0 && (!rows || !row_lane))) {
        ctx->err = "lanes to grid: bad arguments";
        return -1;
    }
    for (int k = 0; k < S; ++k)
        if (views[k].px < 1) { ctx->err = "lanes to grid: px must be at least 1"; return -1; }
    if (S == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    PCA_CHECK(ctx, hipSetDevice(ctx->device));
    if (P < 2 || L == 0) {                                    // no edge anywhere: empty results, no launch
        PCA_CHECK(ctx, hipMemsetAsync(n_rows, 0, sizeof(int64_t) * S, s));
        return 0;
    }
    if (!ws) { ctx->err = "lanes to grid: no workspace"; return -1; }
    const LnWsLayout l = ln_ws_layout(P, S);
    // the views travel through the context's pinned block (free again once the fetch of the call before has run)
    const int64_t vbytes = (int64_t)sizeof(LnView) * S;
    if (ctx->k1n_busy) { PCA_CHECK(ctx, hipEventSynchronize(ctx->k1n_ev)); ctx->k1n_busy = false; }
    if (vbytes > ctx->k1n_pin_cap) {
        if (ctx->k1n_pin) PCA_CHECK(ctx, hipHostFree(ctx->k1n_pin));
        ctx->k1n_pin = nullptr; ctx->k1n_pin_cap = 0;
        PCA_CHECK(ctx, hipHostMalloc(&ctx->k1n_pin, (size_t)(2 * vbytes), hipHostMallocMapped));
        ctx->k1n_pin_cap = 2 * vbytes;
    }
    if (!ctx->k1n_ev) PCA_CHECK(ctx, hipEventCreateWithFlags(&ctx->k1n_ev, hipEventDisableTiming));
    LnView *hv = reinterpret_cast<LnView *>(ctx->k1n_pin);
    for (int k = 0; k < S; ++k) {
        for (int i = 0; i < 3; ++i) hv[k].origin[i] = views[k].origin[i];
        for (int i = 0; i < 9; ++i) hv[k].R[i] = views[k].R[i];
        hv[k].dx = views[k].dx; hv[k].dy = views[k].dy; hv[k].view = views[k].view; hv[k].px = (double)views[k].px;
    }
    char *w = reinterpret_cast<char *>(ws);
    if (pca_fetch_block(ctx, ctx->k1n_pin, 0, w + l.views, vbytes, s)) return -1;
    PCA_CHECK(ctx, hipEventRecord(ctx->k1n_ev, s));
    ctx->k1n_busy = true;
    LnArgs a;
    a.xyz = xyz; a.vlane = vertex_lane; a.n_edges = P - 1; a.tiles = l.tiles;
    a.views = reinterpret_cast<const LnView *>(w + l.views);
    a.tile_rows = reinterpret_cast<uint32_t *>(w + l.tile_rows);
    a.cap = cap_rows; a.rows = rows; a.row_lane = row_lane; a.n_rows = n_rows;
    a.status = ctx->ticket + 1;
    hipLaunchKernelGGL(lanes_count, dim3((unsigned)l.tiles, (unsigned)S), dim3(LN_BLK), 0, s, a);
    hipLaunchKernelGGL(lanes_scan, dim3((unsigned)S), dim3(LN_BLK), 0, s, a);
    hipLaunchKernelGGL(lanes_emit, dim3((unsigned)l.tiles, (unsigned)S), dim3(LN_BLK), 0, s, a);
    PCA_CHECK(ctx, hipGetLastError());
    return 0;
}
