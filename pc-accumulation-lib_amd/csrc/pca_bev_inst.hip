// pca_bev_inst.hip -- the object voxels of the BEV window clustered into instances: connected-component labelling of the voxel
// pass's counts, a deterministic numbering, and the instance of every stored point.  The kept points and their voxels are
// those of pca_bev_voxel_labels: levels 1 and 2 of pca_bev_voxel.hip run first (counts only, into the workspace), and the point
// pass recomputes a point's voxel with the ONE copy of the key in pca_bev_voxel.h.
//
// A call enqueues the two voxel levels and the ten launches below, whatever the data, and never waits for the device.  No
// kernel waits for another workgroup: every loop is bounded by its data or is a lock-free retry that some lane always wins.
// The kernels over the grid are 256 threads, one voxel per thread and round, G workgroups that stride over the grid.
//
//   bev_inst_init      parent[v] = v where counts[v] >= min_points, else -1; size[v] = 0; the foreground count (stats[1]).
//   bev_inst_merge     union-find without iteration to convergence, in two phases with a compress between them.  Phase 0:
//                      every foreground voxel unites with the voxel before it in its row; phase 1: with the rest of the
//                      BACKWARD half of its neighbourhood (2 places of 3 at 6-connectivity, 12 of 13 at 26).  unite(a, b) =
//                      find, find, atomicMin on the larger root, repeated from the value that returns: always larger ->
//                      smaller, so a component's root is its smallest place.  The loads of parent are relaxed agent-scope
//                      atomic loads (the L2s of the XCDs are not coherent for plain ones); a stale root only costs a retry.
//                      Nothing wraps: each neighbour is bounds-checked per coordinate.
//   bev_inst_compress  parent[v] = find(v) (plain loads: nothing else writes; a value another thread has compressed is an
//                      ancestor still).  After phase 0 every voxel points at the first voxel of its row run, which keeps the
//                      chains of phase 1 short; after phase 1, with `count`, size[root] += 1 per voxel, aggregated as below.
//   bev_inst_sums      scan, part 1: tiles of 4 096 voxels; partial[tile] = the surviving roots in it (parent[v] == v and
//                      size[v] >= min_voxels); the roots (stats[2]) and the largest surviving size (stats[5]).
//   bev_inst_offsets   scan, part 2: ONE workgroup, the exclusive prefix sum over the at most 8 192 partials, in place; the
//                      total is n (stats[3]).  Decoupled: no workgroup looks back at, or waits for, another.
//   bev_inst_number    scan, part 3: a thread owns 16 consecutive voxels of its tile, wave scan, LDS across the waves, plus the
//                      tile's offset: the id of a surviving root = the surviving roots at smaller places.  size[v] becomes
//                      that id (else -1) and row id of the table its root, size and the identities of its extremes.
//   bev_inst_write     inst[v] = id of parent[v]; the six extremes by atomicMin / atomicMax on the table, aggregated as below.
//   bev_inst_points    one thread per window point: the key, ids[p] = inst[voxel] (or -1), and the adds on table[id].points and
//                      label_counts[id][label], aggregated as below.  Its window is pca_point_pass.h's, as are the counters
//                      of init, sums and points (point_count).
// Aggregation (compress, write, points): on the headline window, whose classes are uniform, ONE component takes 390 000 voxels
// and 450 000 points, and one global atomic per voxel or point on its row serialises (4.4 + 2.1 + 1.7 ms of a call of 8.7 ms
// without it).  So the lanes of a wave that share a key are counted by ballot (or reduced with the wave's min / max) and their
// first lane alone goes on (inst_for_each_key: a loop over the wave's distinct keys), into a direct-mapped cache of 64 slots
// in the workgroup's LDS (InstSlots: a key claims its slot by compare-and-swap, a key that finds its slot taken goes to global
// memory directly); the slots are flushed once, by the kernel's last lines.
// All sums are integer sums and all extremes integer extremes: the result does not depend on any order.
// Scope: the boxes are voxel boxes (the metric box tighter than the voxels: pca_bev_boxes.hip); the tile-local LDS stage for the
// merge is not built (profiles/bev_voxel_instances.txt has the plain form's time).  The store is never written.
#include "pca_bev_voxel.h"
#include "pca_point_pass.h"

#define INST_THREADS POINT_THREADS // (with POINT_MAX_G the one pair of pca_point_pass.h, for every kernel but bev_inst_offsets)
#define INST_TILE 4096            // voxels per scan tile: 16 per thread
#define INST_PER (INST_TILE / INST_THREADS)

struct alignas(16) InstArgs {
    VoxArgs v;
    int64_t cells;                // nz px px
    int conn;                     // 6 or 26
    int G, Gp;                    // workgroups of the grid kernels / of bev_inst_points
    int tiles;                    // scan tiles
    uint32_t min_points, min_voxels, max_instances;
    uint32_t *counts;             // [cells]: the voxel pass's
    int32_t *parent;              // [cells]: -1 background, else a smaller-or-equal place of the same component
    uint32_t *size;               // [cells]: voxels per root; from bev_inst_number on the id of a surviving root, else -1
    uint32_t *partial;            // [tiles]
    int32_t *inst;                // [cells]: the output, or its stand-in in the workspace
    int32_t *ids;                 // [window points] or NULL
    uint32_t *table;              // [max_instances][PCA_BEV_INST_COLS] or NULL
    uint32_t *label_counts;       // [max_instances][n_labels] or NULL
    unsigned long long *stats;    // [6] or NULL
};

__device__ __forceinline__ int32_t inst_load(const int32_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int32_t inst_find(const int32_t *parent, int32_t x)
{
    for (int32_t p = inst_load(parent + x); p != x; p = inst_load(parent + x)) x = p;   // (p < x: bounded by the place)
    return x;
}
// lock-free: a loser of the atomicMin goes on from what the winner wrote, which is smaller
__device__ __forceinline__ void inst_unite(int32_t *parent, int32_t a, int32_t b)
{
    for (;;) {
        a = inst_find(parent, a);
        b = inst_find(parent, b);
        if (a == b) return;
        if (a < b) { const int32_t t = a; a = b; b = t; }  // a: the larger root
        const int32_t old = atomicMin(parent + a, b);
        if (old == a) return;                               // a was a root still: linked
        a = old;                                            // somebody linked a first: unite what it wrote with b
    }
}
// (inst_for_each_key and InstSlots, the wave and workgroup aggregation in front of the hot rows: pca_point_pass.h)

__global__ __launch_bounds__(INST_THREADS) void bev_inst_init(const InstArgs a)
{
    uint32_t n = 0;
    for (int64_t v = (int64_t)blockIdx.x * INST_THREADS + threadIdx.x; v < a.cells; v += (int64_t)a.G * INST_THREADS) {
        const bool fg = pca_ldg(a.counts + v) >= a.min_points;
        a.parent[v] = fg ? (int32_t)v : -1;
        a.size[v] = 0;
        n += fg;
    }
    point_count(a.stats ? a.stats + 1 : nullptr, n);
}

template <int PHASE>
__global__ __launch_bounds__(INST_THREADS) void bev_inst_merge(const InstArgs a)
{
    const int px = a.v.s.prm.px, nz = a.v.nz;
    const int64_t plane = (int64_t)px * px;
    for (int64_t v = (int64_t)blockIdx.x * INST_THREADS + threadIdx.x; v < a.cells; v += (int64_t)a.G * INST_THREADS) {
        if (inst_load(a.parent + v) < 0) continue;          // (foreground stays foreground: only places are ever written)
        const int k = (int)(v / plane), row = (int)((v - k * plane) / px), col = (int)(v - k * plane - (int64_t)row * px);
        if (PHASE == 0) {
            if (col > 0 && inst_load(a.parent + v - 1) >= 0) inst_unite(a.parent, (int32_t)v, (int32_t)(v - 1));
            continue;
        }
#pragma unroll
        for (int dk = -1; dk <= 0; ++dk)
#pragma unroll
            for (int dr = -1; dr <= 1; ++dr)
#pragma unroll
                for (int dc = -1; dc <= 1; ++dc) {
                    if (dk == 0 && (dr > 0 || (dr == 0 && dc >= -1))) continue;     // the backward half, less phase 0's place
                    const bool face = (dk != 0) + (dr != 0) + (dc != 0) == 1;
                    if (!face && a.conn == 6) continue;
                    const int kk = k + dk, rr = row + dr, cc = col + dc;
                    if (kk < 0 || kk >= nz || rr < 0 || rr >= px || cc < 0 || cc >= px) continue;   // nothing wraps
                    const int64_t u = kk * plane + (int64_t)rr * px + cc;
                    if (inst_load(a.parent + u) >= 0) inst_unite(a.parent, (int32_t)v, (int32_t)u);
                }
    }
}

__global__ __launch_bounds__(INST_THREADS) void bev_inst_compress(const InstArgs a, int count)
{
    __shared__ InstSlots s_slots;
    inst_slots_init(s_slots, false);
    const int64_t rounds = (a.cells + (int64_t)a.G * INST_THREADS - 1) / ((int64_t)a.G * INST_THREADS);
    for (int64_t r = 0; r < rounds; ++r) {                  // (every lane goes round: the ballots need them all)
        const int64_t v = (r * a.G + blockIdx.x) * INST_THREADS + threadIdx.x;
        int32_t x = v < a.cells ? a.parent[v] : -1;
        if (x >= 0) {
            for (int32_t p = a.parent[x]; p != x; p = a.parent[x]) x = p;
            a.parent[v] = x;
        }
        if (!count) continue;
        // size[root] += the wave's voxels of that root: one add per wave and root, into the workgroup's slot where it has one
        inst_for_each_key((uint32_t)x, [&](uint32_t root, unsigned long long lanes, bool leader) {
            if (!leader) return;
            const uint32_t n = (uint32_t)__popcll(lanes);
            const int slot = inst_slots_claim(s_slots, root);
            if (slot >= 0) atomicAdd(&s_slots.val[slot][0], n); else atomicAdd(a.size + root, n);
        });
    }
    __syncthreads();
    if (count && threadIdx.x < INST_SLOTS && s_slots.key[threadIdx.x] != 0xffffffffu)
        atomicAdd(a.size + s_slots.key[threadIdx.x], s_slots.val[threadIdx.x][0]);
}

__global__ __launch_bounds__(INST_THREADS) void bev_inst_sums(const InstArgs a)
{
    __shared__ uint32_t s_w[INST_THREADS / 64];
    const int tid = (int)threadIdx.x;
    uint32_t n_roots = 0, largest = 0;
    for (int tile = (int)blockIdx.x; tile < a.tiles; tile += a.G) {
        uint32_t n = 0;
        for (int i = 0; i < INST_PER; ++i) {
            const int64_t v = (int64_t)tile * INST_TILE + i * INST_THREADS + tid;
            if (v >= a.cells || pca_ldg(a.parent + v) != (int32_t)v) continue;
            ++n_roots;
            const uint32_t sz = pca_ldg(a.size + v);
            if (sz >= a.min_voxels) { ++n; largest = sz > largest ? sz : largest; }
        }
        const uint32_t w = wave_reduce_add(n);
        if ((tid & 63) == 0) s_w[tid >> 6] = w;
        __syncthreads();
        if (tid == 0) a.partial[tile] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
        __syncthreads();
    }
    point_count(a.stats ? a.stats + 2 : nullptr, n_roots);
    const uint32_t w_largest = wave_reduce_max(largest);
    if ((tid & 63) == 0 && a.stats && w_largest) atomicMax(a.stats + 5, (unsigned long long)w_largest);
}

// ONE workgroup: exclusive prefix sum over partial[0, tiles), in place (tiles <= 8 192: 32 consecutive per thread)
__global__ __launch_bounds__(INST_THREADS) void bev_inst_offsets(const InstArgs a)
{
    __shared__ uint32_t s_w[INST_THREADS / 64];
    const int tid = (int)threadIdx.x;
    const int per = (a.tiles + INST_THREADS - 1) / INST_THREADS, t0 = tid * per;
    uint32_t sum = 0;
    for (int i = 0; i < per; ++i) sum += t0 + i < a.tiles ? a.partial[t0 + i] : 0u;
    const uint32_t inc = wave_incl_scan_add(sum);
    if ((tid & 63) == 63) s_w[tid >> 6] = inc;
    __syncthreads();
    uint32_t run = inc - sum;
    for (int k = 0; k < (tid >> 6); ++k) run += s_w[k];
    for (int i = 0; i < per && t0 + i < a.tiles; ++i) {
        const uint32_t c = a.partial[t0 + i];
        a.partial[t0 + i] = run;
        run += c;
    }
    if (tid == 0 && a.stats) a.stats[3] = (unsigned long long)s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

__global__ __launch_bounds__(INST_THREADS) void bev_inst_number(const InstArgs a)
{
    __shared__ uint32_t s_w[INST_THREADS / 64];
    const int tid = (int)threadIdx.x;
    for (int tile = (int)blockIdx.x; tile < a.tiles; tile += a.G) {
        const int64_t v0 = (int64_t)tile * INST_TILE + (int64_t)tid * INST_PER;
        uint32_t flags = 0, sum = 0;
        for (int i = 0; i < INST_PER; ++i) {
            const int64_t v = v0 + i;
            if (v < a.cells && pca_ldg(a.parent + v) == (int32_t)v && pca_ldg(a.size + v) >= a.min_voxels) { flags |= 1u << i; ++sum; }
        }
        const uint32_t inc = wave_incl_scan_add(sum);
        if ((tid & 63) == 63) s_w[tid >> 6] = inc;
        __syncthreads();
        uint32_t id = pca_ldg(a.partial + tile) + inc - sum;
        for (int k = 0; k < (tid >> 6); ++k) id += s_w[k];
        for (int i = 0; i < INST_PER; ++i) {
            const int64_t v = v0 + i;
            if (v >= a.cells) break;
            if (!(flags >> i & 1u)) { a.size[v] = 0xffffffffu; continue; }
            if (a.table && id < a.max_instances) {
                uint32_t *row = a.table + (size_t)id * PCA_BEV_INST_COLS;
                row[0] = (uint32_t)v; row[1] = a.size[v]; row[2] = 0;
                row[3] = 0xffffffffu; row[4] = 0; row[5] = 0xffffffffu; row[6] = 0; row[7] = 0xffffffffu; row[8] = 0;
            }
            a.size[v] = id++;
        }
        __syncthreads();                                    // (the next tile's sums overwrite s_w)
    }
}

__global__ __launch_bounds__(INST_THREADS) void bev_inst_write(const InstArgs a)
{
    __shared__ InstSlots s_slots;
    inst_slots_init(s_slots, true);
    const int px = a.v.s.prm.px;
    const int64_t plane = (int64_t)px * px;
    const int64_t rounds = (a.cells + (int64_t)a.G * INST_THREADS - 1) / ((int64_t)a.G * INST_THREADS);
    for (int64_t r = 0; r < rounds; ++r) {                  // (every lane goes round: the wave reductions need them all)
        const int64_t v = (r * a.G + blockIdx.x) * INST_THREADS + threadIdx.x;
        int32_t id = -1;
        uint32_t k = 0, row = 0, col = 0;
        if (v < a.cells) {
            const int32_t root = pca_ldg(a.parent + v);
            if (root >= 0) id = (int32_t)pca_ldg(a.size + root);
            a.inst[v] = id;
            k = (uint32_t)(v / plane); row = (uint32_t)((v - k * plane) / px); col = (uint32_t)(v - k * plane - (int64_t)row * px);
        }
        if (!a.table) continue;
        const uint32_t key = id >= 0 && (uint32_t)id < a.max_instances ? (uint32_t)id : 0xffffffffu;
        // the extremes of the wave's voxels of one instance, reduced over the wave; its first lane hands them on
        inst_for_each_key(key, [&](uint32_t uid, unsigned long long, bool leader) {
            const bool mine = key == uid;
            uint32_t e[6];
            e[0] = wave_reduce_min(mine ? col : 0xffffffffu); e[1] = wave_reduce_max(mine ? col : 0u);
            e[2] = wave_reduce_min(mine ? row : 0xffffffffu); e[3] = wave_reduce_max(mine ? row : 0u);
            e[4] = wave_reduce_min(mine ? k : 0xffffffffu); e[5] = wave_reduce_max(mine ? k : 0u);
            if (!leader) return;
            const int slot = inst_slots_claim(s_slots, uid);
            uint32_t *t = slot >= 0 ? s_slots.val[slot] : a.table + (size_t)uid * PCA_BEV_INST_COLS + 3;
            for (int j = 0; j < 6; j += 2) { atomicMin(t + j, e[j]); atomicMax(t + j + 1, e[j + 1]); }
        });
    }
    __syncthreads();
    if (a.table && threadIdx.x < INST_SLOTS && s_slots.key[threadIdx.x] != 0xffffffffu) {
        uint32_t *t = a.table + (size_t)s_slots.key[threadIdx.x] * PCA_BEV_INST_COLS + 3;
        for (int j = 0; j < 6; j += 2) { atomicMin(t + j, s_slots.val[threadIdx.x][j]); atomicMax(t + j + 1, s_slots.val[threadIdx.x][j + 1]); }
    }
}

__global__ __launch_bounds__(INST_THREADS) void bev_inst_points(const InstArgs a)
{
    __shared__ uint8_t s_label[256];
    __shared__ InstSlots s_slots;
    const int tid = (int)threadIdx.x;
    s_label[tid] = a.v.label_of[tid];
    inst_slots_init(s_slots, false);
    const SideArgs &s = a.v.s;
    const PointWindow w = point_window<false>(s);          // (cut at max_points as the voxel pass cuts it, which raises the bit)
    const int64_t lo = w.lo, hi = w.hi;
    const PendHi pend_hi = owed_bounds(s.owed, s.frame_off, s.slot_begin, lo);
    const ViewConst vc = view_const(s.prm, s.tx, 0, 0);
    const int px = s.prm.px, nl = a.v.n_labels;
    uint32_t n_kept = 0, n_with = 0;
    for (int64_t c_lo = lo + (int64_t)blockIdx.x * INST_THREADS; c_lo < hi; c_lo += (int64_t)a.Gp * INST_THREADS) {
        const int64_t p = c_lo + tid;
        uint32_t k2 = 0xffffffffu;                          // id << 5 | label of a point that adds to the table
        if (p < hi) {
            const uint32_t key = vox_point_key(a.v, vc, pend_hi, p, s_label);
            int32_t id = -1;
            if (key != KEY_INVALID) {
                ++n_kept;
                id = pca_ldg(a.inst + vox_key_place(key, s.tx, px));
                if (id >= 0) {
                    ++n_with;
                    if ((uint32_t)id < a.max_instances) k2 = ((uint32_t)id << 5) | (key & 31u);
                }
            }
            if (a.ids) a.ids[p - lo] = id;
        }
        if (!a.table && !a.label_counts) continue;
        // lanes of equal (id, label): counted by ballot; their first lane adds the count to the workgroup's slot, or to memory
        inst_for_each_key(k2, [&](uint32_t kk, unsigned long long lanes, bool leader) {
            if (!leader) return;
            const uint32_t n = (uint32_t)__popcll(lanes), id = kk >> 5;
            const int slot = inst_slots_claim(s_slots, kk);
            if (slot >= 0) { atomicAdd(&s_slots.val[slot][0], n); return; }
            if (a.table) atomicAdd(a.table + (size_t)id * PCA_BEV_INST_COLS + 2, n);
            if (a.label_counts) atomicAdd(a.label_counts + (size_t)id * nl + (kk & 31u), n);
        });
    }
    __syncthreads();
    if (tid < INST_SLOTS && s_slots.key[tid] != 0xffffffffu) {
        const uint32_t kk = s_slots.key[tid], n = s_slots.val[tid][0], id = kk >> 5;
        if (a.table) atomicAdd(a.table + (size_t)id * PCA_BEV_INST_COLS + 2, n);
        if (a.label_counts) atomicAdd(a.label_counts + (size_t)id * nl + (kk & 31u), n);
    }
    point_count(a.stats, n_kept);
    point_count(a.stats ? a.stats + 4 : nullptr, n_with);
}

static const WindowPass INST_PASS = {"bev voxel instances", true, false};

// the workspace: the voxel pass's, then counts, parent, size, inst's stand-in and the partials, each at a 256-byte boundary
struct InstLayout { int64_t vox_bytes, counts, parent, size, inst, partial, total; int tiles; };
static inline InstLayout inst_layout(int64_t max_points, int px, int nz)
{
    px = px < 1 ? 1 : (px > SIDE_PX_MAX ? SIDE_PX_MAX : px);
    nz = nz < 1 ? 1 : (nz > PCA_BEV_VOXEL_MAX_Z ? PCA_BEV_VOXEL_MAX_Z : nz);
    const int64_t cells = (int64_t)nz * px * px;
    InstLayout l;
    l.tiles = (int)((cells + INST_TILE - 1) / INST_TILE);
    l.vox_bytes = pca_align256(bev_voxel_workspace(max_points, px));
    l.counts = l.vox_bytes;
    l.parent = l.counts + pca_align256(cells * 4);
    l.size = l.parent + pca_align256(cells * 4);
    l.inst = l.size + pca_align256(cells * 4);
    l.partial = l.inst + pca_align256(cells * 4);
    l.total = l.partial + pca_align256((int64_t)l.tiles * 4) + 256;     // (+ 256: the base is aligned up)
    return l;
}

extern "C" {

int64_t pca_bev_instances_workspace_bytes(int64_t max_points, int px, int nz, int max_instances)
{
    (void)max_instances;                                    // (the table and label_counts are the caller's own)
    return inst_layout(max_points, px, nz).total;
}

int pca_bev_voxel_instances(pca_ctx *ctx, const pca_store *store, const int64_t *frame_off, int slot_begin, int slot_end,
                            int64_t max_points, const pca_bev_params *prm, double z_lo, double z_step, int nz,
                            const uint8_t label_of[256], int n_labels, int dyn_mode, int min_points, int connectivity,
                            int min_voxels, int max_instances, const double *pending_Ts, const int *pending_slot_ends,
                            int n_pending, void *workspace, int64_t workspace_bytes, int32_t *inst, int32_t *ids,
                            uint32_t *table, uint32_t *label_counts, int64_t *stats, void *stream)
{
    if (!ctx) return -1;
    if (max_points < 1) max_points = 1;
    hipStream_t s = (hipStream_t)stream;
    // every check comes before the first launch (a noted K1 and the clearing of the outputs included)
    const std::string w(INST_PASS.what);
    InstArgs A;
    if (max_points >= (1ll << 31)) { ctx->err = w + ": max_points must be below 2^31 (ids and places are 32 bits wide)"; return -1; }
    const bool grid_ok = prm && prm->px >= 1 && prm->px <= SIDE_PX_MAX && nz >= 1 && nz <= PCA_BEV_VOXEL_MAX_Z;
    const InstLayout l = inst_layout(max_points, grid_ok ? prm->px : 1, grid_ok ? nz : 1);
    char *base = reinterpret_cast<char *>(pca_align256(reinterpret_cast<intptr_t>(workspace)));
    if (bev_voxel_prepare(ctx, INST_PASS, inst || ids || table || label_counts || stats, store, frame_off, slot_begin, slot_end,
                          max_points, prm, z_lo, z_step, nz, label_of, n_labels, dyn_mode, pending_Ts, pending_slot_ends, n_pending,
                          base, workspace_bytes < l.total ? 0 : l.vox_bytes, A.v))
        return -1;
    if (dyn_mode < 0 || dyn_mode > 2) { ctx->err = w + ": dyn_mode must be 0, 1 or 2"; return -1; }
    if (min_points < 1) { ctx->err = w + ": min_points must be >= 1"; return -1; }
    if (connectivity != 6 && connectivity != 26) { ctx->err = w + ": connectivity must be 6 or 26"; return -1; }
    if (min_voxels < 1) { ctx->err = w + ": min_voxels must be >= 1"; return -1; }
    if (max_instances < 1 || max_instances > 65536) { ctx->err = w + ": max_instances must be in 1..65536"; return -1; }
    A.cells = (int64_t)nz * prm->px * prm->px;
    A.conn = connectivity;
    A.G = point_pass_G(A.cells, "PCA_BEV_INST_G");          // (one voxel per thread and round: the grid's chunks, the same cap)
    A.Gp = point_pass_G(max_points, "PCA_BEV_INST_G");
    A.tiles = l.tiles;
    A.min_points = (uint32_t)min_points; A.min_voxels = (uint32_t)min_voxels; A.max_instances = (uint32_t)max_instances;
    A.counts = reinterpret_cast<uint32_t *>(base + l.counts);
    A.parent = reinterpret_cast<int32_t *>(base + l.parent);
    A.size = reinterpret_cast<uint32_t *>(base + l.size);
    A.partial = reinterpret_cast<uint32_t *>(base + l.partial);
    A.inst = inst ? inst : reinterpret_cast<int32_t *>(base + l.inst);
    A.ids = ids; A.table = table; A.label_counts = label_counts;
    A.stats = reinterpret_cast<unsigned long long *>(stats);
    A.v.counts = A.counts;
    PCA_CHECK(ctx, hipSetDevice(ctx->device));
    if (bev_voxel_enqueue(ctx, A.v, s)) return -1;          // (a noted K1 runs on its own first; an empty window: counts 0)
    if (table) PCA_CHECK(ctx, hipMemsetAsync(table, 0, (size_t)max_instances * PCA_BEV_INST_COLS * sizeof(uint32_t), s));
    if (label_counts) PCA_CHECK(ctx, hipMemsetAsync(label_counts, 0, (size_t)max_instances * n_labels * sizeof(uint32_t), s));
    if (stats) PCA_CHECK(ctx, hipMemsetAsync(stats, 0, 6 * sizeof(int64_t), s));
    const InstArgs &args = A;
    const dim3 g(args.G), t(INST_THREADS);
    const int tg = args.tiles > args.G ? args.G : args.tiles;
    PCA_LAUNCH(ctx, PCA_K_BEV_INST_INIT, bev_inst_init, g, t, s, args);
    PCA_LAUNCH(ctx, PCA_K_BEV_INST_MERGE, bev_inst_merge<0>, g, t, s, args);
    PCA_LAUNCH(ctx, PCA_K_BEV_INST_COMPRESS, bev_inst_compress, g, t, s, args, 0);
    PCA_LAUNCH(ctx, PCA_K_BEV_INST_MERGE, bev_inst_merge<1>, g, t, s, args);
    PCA_LAUNCH(ctx, PCA_K_BEV_INST_COMPRESS, bev_inst_compress, g, t, s, args, 1);
    PCA_LAUNCH(ctx, PCA_K_BEV_INST_SUMS, bev_inst_sums, dim3(tg), t, s, args);
    PCA_LAUNCH(ctx, PCA_K_BEV_INST_OFFSETS, bev_inst_offsets, dim3(1), t, s, args);
    PCA_LAUNCH(ctx, PCA_K_BEV_INST_NUMBER, bev_inst_number, dim3(tg), t, s, args);
    PCA_LAUNCH(ctx, PCA_K_BEV_INST_WRITE, bev_inst_write, g, t, s, args);
    if (slot_end > slot_begin)                              // (a window without a slot: no launch over zero points)
        PCA_LAUNCH(ctx, PCA_K_BEV_INST_POINTS, bev_inst_points, dim3(args.Gp), t, s, args);
    PCA_CHECK(ctx, hipGetLastError());
    return 0;
}

}  // extern "C"
