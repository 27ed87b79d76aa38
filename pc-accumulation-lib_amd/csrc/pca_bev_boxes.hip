// pca_bev_boxes.hip -- oriented metric boxes around the window's instances (pca_bev_instance_boxes): per instance id and per
// direction of the caller's table, the rectangle around the instance's points; then the direction chosen by area or by the
// number of points near an edge.  The window, its cuts and the counters are pca_point_pass.h's; the coordinates are the view
// test's own expressions (pca_bev_view.h), so a point's box coordinates are the ones its cell came from.
//
// A call enqueues the launches below, whatever the data, and never waits for the device.  No kernel waits for another
// workgroup.  256 threads except where said.
//
//   bev_box_table    the caller's HOST table of directions reaches the device as a kernel argument, 128 directions a launch
//                    (a copy command from pageable memory may wait for the stream; a launch does not).
//   bev_box_count    one thread per window point over ids alone: count[id] += 1 where 0 <= id < n_rows, aggregated per wave
//                    by ballot and per workgroup in LDS slots (inst_for_each_key, InstSlots); stats 0 and 1; the overflow bit.
//   bev_box_offsets  ONE workgroup of 1 024 threads: the exclusive scan of the row counts (tiles of 4 096 rows), which
//                    also gives the table of PIECES: a row of n points is cut into ceil(n / 2048) of them.  There are at most
//                    max_points / 2048 + n_rows pieces, so the grids behind are sized without reading anything back.
//                    stats 2 and 3.
//   bev_box_scatter  one thread per window point, 1 024 a workgroup: (ax, ay, z) of a point that takes part, into its row's segment
//                    through the row's cursor -- one atomic add per WORKGROUP, chunk and row (ballot ranks, LDS slots).  The order
//                    inside a segment is arbitrary and does not matter: only extremes and counts are taken from it.
//   bev_box_walk<0>  the extents.  Workgroups stride over the pieces; a piece's (ax, ay) are staged in LDS (32 KiB).  A LANE
//                    OWNS A DIRECTION, not a point: it walks the piece's points as LDS broadcast reads and keeps its four
//                    extremes in registers, so no cross-lane reduction is needed per direction.  With fewer directions than
//                    threads the point range is dealt to 256 / n_angles lane groups, combined in LDS.  A row of one piece
//                    stores; a row of several pieces combines by 64-bit atomic min / max on an order-preserving encoding of
//                    the f64 (the start values are two memsets: 0xff for the minima, 0 for the maxima).  z the same way.
//   bev_box_walk<1>  near_t: the same walk against the finished extents, integer adds.  Enqueued iff near_t is needed.
//   bev_box_choose   a wave per row, a lane per direction (in rounds of 64): the best direction by the criterion, a total
//                    order, reduced over the wave; writes fit, fit_n and the decoded extents.
// Scope: boxes stand on the ground plane; nothing is tracked, merged or split; no variance criterion (float sums would depend
// on the order); no label file is written.  The store is never written.
#include "pca_point_pass.h"

#define BOX_THREADS POINT_THREADS
#define BOX_WIDE 1024             // threads of bev_box_offsets and bev_box_scatter
#define BOX_PIECE 2048            // points of a piece: 32 KiB of (ax, ay) in LDS
#define BOX_TABLE_PER 128         // directions per bev_box_table launch (2 KiB of kernel arguments)
#define BOX_MAX_ROWS 65536
#define BOX_MAX_ANGLES 256

struct alignas(16) BoxArgs {
    pca_store st;
    const int64_t *frame_off;
    int slot_begin, slot_end;
    int64_t max_points;
    pca_bev_params prm;
    BevOwed owed;                 // owed re-transforms: applied to the points that are read, never written back
    uint32_t *status;             // context status word (PCA_STATUS_* bits)
    const int32_t *ids;           // [window points]
    int n_rows, n_angles, criterion, want_near;
    double edge_dist;
    int G, Gw, Gs, Gc;            // workgroups of bev_box_count / bev_box_scatter / the walks over the pieces / bev_box_choose
    int max_pieces;
    const double *cs;             // [n_angles][2], the device copy
    uint32_t *count, *offset, *piece_first, *cursor;    // [n_rows] each: points, first point, first piece, next free place
    uint32_t *piece_row;          // [max_pieces]
    uint32_t *n_pieces;           // [1]
    double *px, *py, *pz;         // [max_points] each: ax, ay, z of the points that take part, row after row
    unsigned long long *mins, *maxs;   // encoded [n_rows][n_angles][2] (e1, e2), then [n_rows] (z)
    uint32_t *near_acc;           // [n_rows][n_angles]: the output, or its stand-in in the workspace (want_near)
    double *fit;                  // [n_rows][8] or NULL
    uint32_t *fit_n;              // [n_rows][2] or NULL
    double *extents;              // [n_rows][n_angles][4] or NULL
    unsigned long long *stats;    // [4] or NULL
};
struct BoxTable { double v[BOX_TABLE_PER * 2]; };

// f64 <-> u64, order-preserving (a < b <=> enc(a) < enc(b) for numbers; -0.0 never occurs: every value had + 0.0)
__device__ __forceinline__ unsigned long long box_enc(double d)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(d);
    return u ^ ((u >> 63) ? ~0ull : (1ull << 63));
}
__device__ __forceinline__ double box_dec(unsigned long long e)
{
    return __longlong_as_double((long long)(e ^ ((e >> 63) ? (1ull << 63) : ~0ull)));
}

__global__ __launch_bounds__(BOX_THREADS) void bev_box_table(const BoxTable t, double *cs, int n)
{
    const int i = (int)threadIdx.x;
    if (i < n) cs[i] = t.v[i];
}

// the row of point p of the window, or 0xffffffff; n_over: ids behind the rows
__device__ __forceinline__ uint32_t box_key(const BoxArgs &a, int64_t p, int64_t lo, int64_t hi, uint32_t &n_over)
{
    if (p >= hi) return 0xffffffffu;
    const int32_t id = pca_ldg(a.ids + (p - lo));
    if (id < 0) return 0xffffffffu;
    if (id >= a.n_rows) { ++n_over; return 0xffffffffu; }
    return (uint32_t)id;
}

__global__ __launch_bounds__(BOX_THREADS) void bev_box_count(const BoxArgs a)
{
    __shared__ InstSlots s_slots;
    inst_slots_init(s_slots, false);
    const int tid = (int)threadIdx.x;
    const PointWindow w = point_window<true>(a);
    const int64_t lo = w.lo, hi = w.hi;
    uint32_t n_part = 0, n_over = 0;
    for (int64_t c_lo = lo + (int64_t)blockIdx.x * BOX_THREADS; c_lo < hi; c_lo += (int64_t)a.G * BOX_THREADS) {
        const uint32_t key = box_key(a, c_lo + tid, lo, hi, n_over);
        n_part += key != 0xffffffffu;
        inst_for_each_key(key, [&](uint32_t row, unsigned long long lanes, bool leader) {
            if (!leader) return;
            const uint32_t n = (uint32_t)__popcll(lanes);
            const int slot = inst_slots_claim(s_slots, row);
            if (slot >= 0) atomicAdd(&s_slots.val[slot][0], n); else atomicAdd(a.count + row, n);
        });
    }
    __syncthreads();
    if (tid < INST_SLOTS && s_slots.key[tid] != 0xffffffffu) atomicAdd(a.count + s_slots.key[tid], s_slots.val[tid][0]);
    point_count(a.stats, n_part, n_over);
}

// ONE workgroup of 1 024 threads: offset, cursor and piece_first of every row, the table of pieces and their number.  Tiles of
// 4 096 rows, four consecutive rows per thread (a wave reads and writes whole lines), the running totals carried in registers.
__global__ __launch_bounds__(BOX_WIDE) void bev_box_offsets(const BoxArgs a)
{
    __shared__ uint32_t s_pts[BOX_WIDE / 64], s_pcs[BOX_WIDE / 64];
    const int tid = (int)threadIdx.x, wave = tid >> 6;
    uint32_t run_pts = 0, run_pcs = 0, n_used = 0, largest = 0;
    for (int base = 0; base < a.n_rows; base += BOX_WIDE * 4) {
        const int r0 = base + tid * 4;
        uint32_t c[4], pts = 0, pcs = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            c[i] = r0 + i < a.n_rows ? a.count[r0 + i] : 0u;
            pts += c[i];
            pcs += (c[i] + BOX_PIECE - 1) / BOX_PIECE;
            n_used += c[i] != 0;
            largest = c[i] > largest ? c[i] : largest;
        }
        const uint32_t inc_pts = wave_incl_scan_add(pts), inc_pcs = wave_incl_scan_add(pcs);
        if ((tid & 63) == 63) { s_pts[wave] = inc_pts; s_pcs[wave] = inc_pcs; }
        __syncthreads();
        uint32_t my_pts = run_pts + inc_pts - pts, my_pcs = run_pcs + inc_pcs - pcs;
        for (int k = 0; k < BOX_WIDE / 64; ++k) {
            if (k < wave) { my_pts += s_pts[k]; my_pcs += s_pcs[k]; }
            run_pts += s_pts[k]; run_pcs += s_pcs[k];       // (every thread carries the same totals)
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = r0 + i;
            if (r >= a.n_rows) break;
            const uint32_t n = (c[i] + BOX_PIECE - 1) / BOX_PIECE;
            a.offset[r] = my_pts; a.cursor[r] = my_pts; a.piece_first[r] = my_pcs;
            for (uint32_t k = 0; k < n; ++k)
                if (my_pcs + k < (uint32_t)a.max_pieces) a.piece_row[my_pcs + k] = (uint32_t)r;     // (always: pieces <= max_points / 2048 + n_rows)
            my_pts += c[i]; my_pcs += n;
        }
        __syncthreads();                                    // (the next tile's sums overwrite s_pts, s_pcs)
    }
    if (tid == 0) *a.n_pieces = run_pcs < (uint32_t)a.max_pieces ? run_pcs : (uint32_t)a.max_pieces;
    point_count(a.stats ? a.stats + 2 : nullptr, n_used);
    const uint32_t w_largest = wave_reduce_max(largest);
    if ((tid & 63) == 0 && a.stats && w_largest) atomicMax(a.stats + 3, (unsigned long long)w_largest);
}

// 1 024 threads, chunks of 1 024 points: per chunk ONE add on a row's cursor from the whole workgroup (the wave's lanes of a row
// are ranked by ballot, the waves' counts meet in the row's LDS slot, the slot's owner adds their sum), so the one row that holds
// most of a window does not serialise a global atomic per wave (headline window: 502 us with one add per wave, 45 us so).
__global__ __launch_bounds__(BOX_WIDE) void bev_box_scatter(const BoxArgs a)
{
    __shared__ InstSlots s_slots;                           // val[0]: the chunk's points of the slot's row, val[1]: where they start
    const int tid = (int)threadIdx.x;
    const PointWindow w = point_window<false>(a);
    const int64_t lo = w.lo, hi = w.hi;
    const PendHi pend_hi = owed_bounds(a.owed, a.frame_off, a.slot_begin, lo);
    const double ox = a.prm.origin[0], oy = a.prm.origin[1], oz = a.prm.origin[2];
    const double r0 = a.prm.R[0], r1 = a.prm.R[1], r3 = a.prm.R[3], r4 = a.prm.R[4], dx = a.prm.dx, dy = a.prm.dy;
    const unsigned long long below = (1ull << (tid & 63)) - 1ull;
    for (int64_t c_lo = lo + (int64_t)blockIdx.x * BOX_WIDE; c_lo < hi; c_lo += (int64_t)a.Gw * BOX_WIDE) {
        inst_slots_init(s_slots, false);
        const int64_t p = c_lo + tid;
        uint32_t n_over = 0;
        const uint32_t key = box_key(a, p, lo, hi, n_over);
        double ax = 0.0, ay = 0.0, z = 0.0;
        if (key != 0xffffffffu) {
            double X = pca_ldg(a.st.x + p), Y = pca_ldg(a.st.y + p), Z = pca_ldg(a.st.z + p);
            apply_owed(a.owed, pend_hi, p, X, Y, Z);
            const double x = X - ox, y = Y - oy;            // the expressions of view_key_lean
            ax = fma(r1, y, r0 * x) + dx;
            ay = fma(r4, y, r3 * x) + dy;
            z = (Z - oz) + 0.0;
        }
        // a lane's place = where its wave's share begins (in the row's slot, or -- the slot taken by another row -- on the
        // cursor itself) + its rank among the wave's lanes of the row
        uint32_t pos = 0xffffffffu;
        int slot = -1;
        inst_for_each_key(key, [&](uint32_t row, unsigned long long lanes, bool leader) {
            const uint32_t n = (uint32_t)__popcll(lanes);
            const int first = __ffsll((long long)lanes) - 1;
            int sl = -1;
            uint32_t base = 0;
            if (leader) {
                sl = inst_slots_claim(s_slots, row);
                base = sl >= 0 ? atomicAdd(&s_slots.val[sl][0], n) : atomicAdd(a.cursor + row, n);
            }
            sl = __builtin_amdgcn_readlane(sl, first);
            base = (uint32_t)__builtin_amdgcn_readlane((int)base, first);
            if (key == row) { slot = sl; pos = base + (uint32_t)__popcll(lanes & below); }
        });
        __syncthreads();
        if (tid < INST_SLOTS && s_slots.key[tid] != 0xffffffffu)
            s_slots.val[tid][1] = atomicAdd(a.cursor + s_slots.key[tid], s_slots.val[tid][0]);
        __syncthreads();
        if (slot >= 0) pos += s_slots.val[slot][1];
        if (key != 0xffffffffu && (int64_t)pos < a.max_points) {   // (always: the cursors end where the counts said)
            a.px[pos] = ax; a.py[pos] = ay; a.pz[pos] = z;
        }
        __syncthreads();                                    // (the next chunk clears the slots)
    }
}

// NEAR = 0: the extents of every piece; NEAR = 1: near_t against the finished extents
template <int NEAR>
__global__ __launch_bounds__(BOX_THREADS) void bev_box_walk(const BoxArgs a)
{
    __shared__ double s_x[BOX_PIECE], s_y[BOX_PIECE];
    __shared__ double s_e[BOX_THREADS][4];                  // the lane groups' extremes
    __shared__ uint32_t s_n[BOX_THREADS];                   // ... or their counts
    __shared__ unsigned long long s_z[2];
    const int tid = (int)threadIdx.x;
    const int A = a.n_angles, ng = BOX_THREADS / A;         // lane groups: the point range is dealt to them
    const bool active = tid < ng * A;
    const int d = tid % A, g = tid / A;
    const double c = active ? pca_ldg(a.cs + 2 * d) : 0.0, s = active ? pca_ldg(a.cs + 2 * d + 1) : 0.0;
    const double inf = __builtin_huge_val(), edge = a.edge_dist;
    const uint32_t n_pieces = pca_ldg(a.n_pieces);
    const size_t z_base = (size_t)a.n_rows * A * 2;
    for (uint32_t pc = blockIdx.x; pc < n_pieces; pc += (uint32_t)a.Gs) {
        const uint32_t row = pca_ldg(a.piece_row + pc), cnt = pca_ldg(a.count + row);
        const uint32_t start = pca_ldg(a.offset + row) + (pc - pca_ldg(a.piece_first + row)) * BOX_PIECE;
        const uint32_t left = pca_ldg(a.offset + row) + cnt - start;
        const int m = (int)(left < BOX_PIECE ? left : BOX_PIECE);
        const bool multi = cnt > BOX_PIECE;
        const size_t at = ((size_t)row * A + d) * 2;
        __syncthreads();                                    // (the walk of the piece before has read s_x, s_y, s_e)
        if (!NEAR && tid < 2) s_z[tid] = tid ? 0ull : ~0ull;
        for (int i = tid; i < m; i += BOX_THREADS) { s_x[i] = pca_ldg(a.px + start + i); s_y[i] = pca_ldg(a.py + start + i); }
        __syncthreads();
        if (!NEAR) {
            double zl = inf, zh = -inf;
            for (int i = tid; i < m; i += BOX_THREADS) {
                const double v = pca_ldg(a.pz + start + i);
                zl = v < zl ? v : zl; zh = v > zh ? v : zh;
            }
            if (tid < m) { atomicMin(&s_z[0], box_enc(zl)); atomicMax(&s_z[1], box_enc(zh)); }
            double lo1 = inf, hi1 = -inf, lo2 = inf, hi2 = -inf;
            if (active)
                for (int i = g; i < m; i += ng) {
                    const double x = s_x[i], y = s_y[i];
                    const double e1 = (c * x + s * y) + 0.0, e2 = (c * y - s * x) + 0.0;
                    lo1 = e1 < lo1 ? e1 : lo1; hi1 = e1 > hi1 ? e1 : hi1;
                    lo2 = e2 < lo2 ? e2 : lo2; hi2 = e2 > hi2 ? e2 : hi2;
                }
            s_e[tid][0] = lo1; s_e[tid][1] = hi1; s_e[tid][2] = lo2; s_e[tid][3] = hi2;
            __syncthreads();
            if (tid < A) {
                for (int k = 1; k < ng; ++k) {
                    const double *o = s_e[k * A + tid];
                    lo1 = o[0] < lo1 ? o[0] : lo1; hi1 = o[1] > hi1 ? o[1] : hi1;
                    lo2 = o[2] < lo2 ? o[2] : lo2; hi2 = o[3] > hi2 ? o[3] : hi2;
                }
                if (multi) {
                    atomicMin(a.mins + at, box_enc(lo1)); atomicMin(a.mins + at + 1, box_enc(lo2));
                    atomicMax(a.maxs + at, box_enc(hi1)); atomicMax(a.maxs + at + 1, box_enc(hi2));
                } else {
                    a.mins[at] = box_enc(lo1); a.mins[at + 1] = box_enc(lo2);
                    a.maxs[at] = box_enc(hi1); a.maxs[at + 1] = box_enc(hi2);
                }
            }
            if (tid < 2) {
                unsigned long long *dst = (tid ? a.maxs : a.mins) + z_base + row;
                if (!multi) *dst = s_z[tid];
                else if (tid) atomicMax(dst, s_z[1]);
                else atomicMin(dst, s_z[0]);
            }
        } else {
            uint32_t n = 0;
            if (active) {
                const double lo1 = box_dec(pca_ldg(a.mins + at)), lo2 = box_dec(pca_ldg(a.mins + at + 1));
                const double hi1 = box_dec(pca_ldg(a.maxs + at)), hi2 = box_dec(pca_ldg(a.maxs + at + 1));
                for (int i = g; i < m; i += ng) {
                    const double x = s_x[i], y = s_y[i];
                    const double e1 = (c * x + s * y) + 0.0, e2 = (c * y - s * x) + 0.0;
                    n += (e1 - lo1 <= edge) | (hi1 - e1 <= edge) | (e2 - lo2 <= edge) | (hi2 - e2 <= edge);
                }
            }
            s_n[tid] = n;
            __syncthreads();
            if (tid < A) {
                for (int k = 1; k < ng; ++k) n += s_n[k * A + tid];
                uint32_t *dst = a.near_acc + (size_t)row * A + tid;
                if (multi) atomicAdd(dst, n); else *dst = n;
            }
        }
    }
}

// the choice is a total order: larger key count, then smaller area (NaN as +inf), then smaller t
struct BoxBest { uint32_t kn; double ka; int t; };
__device__ __forceinline__ bool box_better(const BoxBest &x, const BoxBest &y)
{
    return x.kn > y.kn || (x.kn == y.kn && (x.ka < y.ka || (x.ka == y.ka && x.t < y.t)));
}

__global__ __launch_bounds__(BOX_THREADS) void bev_box_choose(const BoxArgs a)
{
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int A = a.n_angles;
    const double inf = __builtin_huge_val(), nan = __builtin_nan("");
    const size_t z_base = (size_t)a.n_rows * A * 2;
    for (int row = (int)blockIdx.x * (BOX_THREADS / 64) + wave; row < a.n_rows; row += a.Gc * (BOX_THREADS / 64)) {
        const uint32_t n = pca_ldg(a.count + row);
        BoxBest best = {0u, inf, 0x7fffffff};
        double b_lo1 = nan, b_hi1 = nan, b_lo2 = nan, b_hi2 = nan, b_area = nan;
        uint32_t b_near = 0;
        for (int t = lane; t < A; t += 64) {
            const size_t at = ((size_t)row * A + t) * 2;
            double lo1 = inf, hi1 = -inf, lo2 = inf, hi2 = -inf;
            if (n) {
                lo1 = box_dec(pca_ldg(a.mins + at)); lo2 = box_dec(pca_ldg(a.mins + at + 1));
                hi1 = box_dec(pca_ldg(a.maxs + at)); hi2 = box_dec(pca_ldg(a.maxs + at + 1));
            }
            if (a.extents) {
                double *e = a.extents + at * 2;
                e[0] = lo1; e[1] = hi1; e[2] = lo2; e[3] = hi2;
            }
            const double area = (hi1 - lo1) * (hi2 - lo2);
            const uint32_t near = a.want_near ? pca_ldg(a.near_acc + (size_t)row * A + t) : 0u;
            const BoxBest cand = {a.criterion == 1 ? near : 0u, area != area ? inf : area, t};
            if (box_better(cand, best)) {
                best = cand;
                b_lo1 = lo1; b_hi1 = hi1; b_lo2 = lo2; b_hi2 = hi2; b_area = area; b_near = near;
            }
        }
        if (!n) {                                           // (wave-uniform)
            if (lane < 8 && a.fit) a.fit[(size_t)row * 8 + lane] = lane == 7 ? -1.0 : nan;
            if (lane < 2 && a.fit_n) a.fit_n[(size_t)row * 2 + lane] = 0u;
            continue;
        }
        BoxBest win = best;
#pragma unroll
        for (int sft = 1; sft < 64; sft <<= 1) {
            BoxBest o;
            o.kn = (uint32_t)__shfl_xor((int)win.kn, sft);
            o.ka = __shfl_xor(win.ka, sft);
            o.t = __shfl_xor(win.t, sft);
            if (box_better(o, win)) win = o;
        }
        if (best.t == win.t) {                              // (one lane: every direction belongs to one lane)
            if (a.fit) {
                double *f = a.fit + (size_t)row * 8;
                f[0] = b_lo1; f[1] = b_hi1; f[2] = b_lo2; f[3] = b_hi2;
                f[4] = box_dec(pca_ldg(a.mins + z_base + row)); f[5] = box_dec(pca_ldg(a.maxs + z_base + row));
                f[6] = b_area; f[7] = (double)win.t;
            }
            if (a.fit_n) { a.fit_n[(size_t)row * 2] = n; a.fit_n[(size_t)row * 2 + 1] = b_near; }
        }
    }
}

static const WindowPass BOX_PASS = {"bev instance boxes", false, false};

// the workspace: the table, the header, the four row tables, the pieces, the three coordinate arrays, the encoded minima and
// maxima and near's stand-in, each at a 256-byte boundary
struct BoxLayout { int64_t cs, n_pieces, count, offset, piece_first, cursor, piece_row, px, py, pz, mins, maxs, near, total, ext_words; int max_pieces; };
static inline BoxLayout box_layout(int64_t max_points, int n_rows, int n_angles)
{
    BoxLayout l;
    l.max_pieces = (int)(max_points / BOX_PIECE + n_rows);
    l.ext_words = (int64_t)n_rows * n_angles * 2 + n_rows;
    l.cs = 0;
    l.n_pieces = l.cs + pca_align256(BOX_MAX_ANGLES * 2 * (int64_t)sizeof(double));
    l.count = l.n_pieces + 256;
    l.offset = l.count + pca_align256((int64_t)n_rows * 4);
    l.piece_first = l.offset + pca_align256((int64_t)n_rows * 4);
    l.cursor = l.piece_first + pca_align256((int64_t)n_rows * 4);
    l.piece_row = l.cursor + pca_align256((int64_t)n_rows * 4);
    l.px = l.piece_row + pca_align256((int64_t)l.max_pieces * 4);
    l.py = l.px + pca_align256(max_points * 8);
    l.pz = l.py + pca_align256(max_points * 8);
    l.mins = l.pz + pca_align256(max_points * 8);
    l.maxs = l.mins + pca_align256(l.ext_words * 8);
    l.near = l.maxs + pca_align256(l.ext_words * 8);
    l.total = l.near + pca_align256((int64_t)n_rows * n_angles * 4) + 256;      // (+ 256: the base is aligned up)
    return l;
}

extern "C" {

int64_t pca_bev_instance_boxes_workspace_bytes(int64_t max_points, int n_rows, int n_angles)
{
    if (max_points < 1) max_points = 1;
    if (max_points >= (1ll << 31) || n_rows < 1 || n_rows > BOX_MAX_ROWS || n_angles < 1 || n_angles > BOX_MAX_ANGLES) return -1;
    return box_layout(max_points, n_rows, n_angles).total;
}

int pca_bev_instance_boxes(pca_ctx *ctx, const pca_store *store, const int64_t *frame_off, int slot_begin, int slot_end,
                           int64_t max_points, const pca_bev_params *prm, const int32_t *ids, int n_rows, const double *cos_sin,
                           int n_angles, int criterion, double edge_dist, const double *pending_Ts, const int *pending_slot_ends,
                           int n_pending, void *workspace, int64_t workspace_bytes, double *fit, uint32_t *fit_n, double *extents,
                           uint32_t *near, int64_t *stats, void *stream)
{
    if (!ctx) return -1;
    if (max_points < 1) max_points = 1;
    hipStream_t s = (hipStream_t)stream;
    // every check comes before the first launch (a noted K1 and the clearing of the outputs included)
    const std::string w(BOX_PASS.what);
    BoxArgs A;
    auto rotation = [&]() -> int { return bev_check_rotation(ctx, BOX_PASS.what, prm); };
    if (window_check_any(ctx, BOX_PASS, prm && ids && cos_sin && workspace && (fit || fit_n || extents || near || stats), store,
                         frame_off, slot_begin, slot_begin, slot_end, max_points, rotation, pending_Ts, pending_slot_ends,
                         n_pending, A))
        return -1;
    A.prm = *prm;
    if (max_points >= (1ll << 31)) { ctx->err = w + ": max_points must be below 2^31 (places in the segments are 32 bits wide)"; return -1; }
    if (n_rows < 1 || n_rows > BOX_MAX_ROWS) { ctx->err = w + ": n_rows must be in 1..65536"; return -1; }
    if (n_angles < 1 || n_angles > BOX_MAX_ANGLES) { ctx->err = w + ": n_angles must be in 1..256"; return -1; }
    if (criterion != 0 && criterion != 1) { ctx->err = w + ": criterion must be 0 or 1"; return -1; }
    if (!(edge_dist >= 0.0 && edge_dist < __builtin_huge_val())) { ctx->err = w + ": edge_dist must be finite and >= 0"; return -1; }
    for (int i = 0; i < 2 * n_angles; ++i)
        if (!(fabs(cos_sin[i]) < __builtin_huge_val())) { ctx->err = w + ": every entry of cos_sin must be finite"; return -1; }
    const BoxLayout l = box_layout(max_points, n_rows, n_angles);
    if (workspace_bytes < l.total) { ctx->err = w + ": workspace too small"; return -1; }
    char *base = reinterpret_cast<char *>(pca_align256(reinterpret_cast<intptr_t>(workspace)));
    const int64_t cap = pca_env_int("PCA_BEV_BOXES_G", POINT_MAX_G, 1, POINT_MAX_G);
    const int64_t row_groups = (n_rows + BOX_THREADS / 64 - 1) / (BOX_THREADS / 64);
    A.ids = ids;
    A.n_rows = n_rows; A.n_angles = n_angles; A.criterion = criterion; A.want_near = criterion == 1 || near;
    A.edge_dist = edge_dist;
    A.G = point_pass_G(max_points, "PCA_BEV_BOXES_G");
    const int64_t wide = (max_points + BOX_WIDE - 1) / BOX_WIDE;
    A.Gw = (int)(wide > cap ? cap : wide);
    A.Gs = (int)(l.max_pieces > cap ? cap : l.max_pieces);
    A.Gc = (int)(row_groups > cap ? cap : row_groups);
    A.max_pieces = l.max_pieces;
    double *cs = reinterpret_cast<double *>(base + l.cs);
    A.cs = cs;
    A.n_pieces = reinterpret_cast<uint32_t *>(base + l.n_pieces);
    A.count = reinterpret_cast<uint32_t *>(base + l.count);
    A.offset = reinterpret_cast<uint32_t *>(base + l.offset);
    A.piece_first = reinterpret_cast<uint32_t *>(base + l.piece_first);
    A.cursor = reinterpret_cast<uint32_t *>(base + l.cursor);
    A.piece_row = reinterpret_cast<uint32_t *>(base + l.piece_row);
    A.px = reinterpret_cast<double *>(base + l.px);
    A.py = reinterpret_cast<double *>(base + l.py);
    A.pz = reinterpret_cast<double *>(base + l.pz);
    A.mins = reinterpret_cast<unsigned long long *>(base + l.mins);
    A.maxs = reinterpret_cast<unsigned long long *>(base + l.maxs);
    A.near_acc = near ? near : reinterpret_cast<uint32_t *>(base + l.near);
    A.fit = fit; A.fit_n = fit_n; A.extents = extents;
    A.stats = reinterpret_cast<unsigned long long *>(stats);
    PCA_CHECK(ctx, hipSetDevice(ctx->device));
    if (pca_k1_flush_pending(ctx)) return -1;               // a noted K1 runs on its own first
    PCA_CHECK(ctx, hipMemsetAsync(A.count, 0, (size_t)n_rows * sizeof(uint32_t), s));
    PCA_CHECK(ctx, hipMemsetAsync(A.mins, 0xff, (size_t)l.ext_words * 8, s));
    PCA_CHECK(ctx, hipMemsetAsync(A.maxs, 0, (size_t)l.ext_words * 8, s));
    if (A.want_near) PCA_CHECK(ctx, hipMemsetAsync(A.near_acc, 0, (size_t)n_rows * n_angles * sizeof(uint32_t), s));
    if (stats) PCA_CHECK(ctx, hipMemsetAsync(stats, 0, 4 * sizeof(int64_t), s));
    const BoxArgs &args = A;
    const dim3 t(BOX_THREADS);
    for (int first = 0; first < n_angles; first += BOX_TABLE_PER) {
        BoxTable tab;
        const int n = (n_angles - first < BOX_TABLE_PER ? n_angles - first : BOX_TABLE_PER) * 2;
        for (int i = 0; i < BOX_TABLE_PER * 2; ++i) tab.v[i] = i < n ? cos_sin[2 * first + i] : 0.0;
        PCA_LAUNCH(ctx, PCA_K_BEV_BOX_TABLE, bev_box_table, dim3(1), t, s, tab, cs + 2 * first, n);
    }
    if (slot_end > slot_begin)                              // (a window without a slot: no launch over zero points)
        PCA_LAUNCH(ctx, PCA_K_BEV_BOX_COUNT, bev_box_count, dim3(args.G), t, s, args);
    PCA_LAUNCH(ctx, PCA_K_BEV_BOX_OFFSETS, bev_box_offsets, dim3(1), dim3(BOX_WIDE), s, args);
    if (slot_end > slot_begin)
        PCA_LAUNCH(ctx, PCA_K_BEV_BOX_SCATTER, bev_box_scatter, dim3(args.Gw), dim3(BOX_WIDE), s, args);
    PCA_LAUNCH(ctx, PCA_K_BEV_BOX_EXTENTS, bev_box_walk<0>, dim3(args.Gs), t, s, args);
    if (args.want_near)
        PCA_LAUNCH(ctx, PCA_K_BEV_BOX_NEAR, bev_box_walk<1>, dim3(args.Gs), t, s, args);
    PCA_LAUNCH(ctx, PCA_K_BEV_BOX_CHOOSE, bev_box_choose, dim3(args.Gc), t, s, args);
    PCA_CHECK(ctx, hipGetLastError());
    return 0;
}

}  // extern "C"
