// pca_voxel_match.hip -- WHICH instance of the previous sample an instance of this one is: two instance volumes (i32 [nz][px][px], -1 =
// none, as pca_bev_voxel_instances leaves `inst`) and a 3 x 4 map M from the continuous voxel index of `cur` to that of `prev` give,
// per pair (a of prev, b of cur), the number C(a, b) of cur voxels of b whose centre lands in a voxel of a; b MATCHES a iff each is the
// other's best partner (largest C, smallest id among equal ones), C >= min_overlap and C >= min_iou (vox_prev[a] + vox_cur[b] - C).  A
// matched b takes a's track, every other b that has a voxel takes a new number from a counter that lives on the device, so a sequence
// chains without a host read.  The call reads volumes: no store, no points.  Integer counts and maxima only: every defined output
// depends on the SET of voxels, not on which workgroup saw them first (the order of `pairs` excepted).
//
// Five launches whatever the volumes hold, no wait on the device or between workgroups:
//
//   voxel_match_init     the pair table's keys to EMPTY, everything else of the workspace to 0.
//   voxel_match_count    a WAVE takes 64 neighbouring col of one line (k, row) of cur, then of prev (a grid-stride loop over both).  cur:
//                        the id b, the image q = M (col + 0.5, row + 0.5, k + 0.5, 1) in f64 -- ((M0 u + M1 v) + M2 w) + M3, each
//                        operation rounded on its own, the library is built with -ffp-contract=off --, IN VIEW iff 0 <= q < (px, px, nz)
//                        on the f64 values (a NaN is out of view), then a = prev[floor q].  Neighbouring voxels of one instance mostly
//                        land in one prev instance, so the wave folds RUNS of equal keys first: a lane is a run's head iff its key
//                        differs from the lane before it (one ballot), and the head alone touches memory, adding the run's length.
//                        vox_cur / in_view fold by b, the pair table by (a, b), vox_prev (the prev half) by a.  The counters of `stats`
//                        are summed in registers and leave a wave as one atomic each.
//                        The pair table is open addressing over cap_pairs slots (a 64-bit key claimed by compare-and-swap, a 32-bit
//                        count beside it), linear probing from a hash of the key, at most cap_pairs probes: then the increment is given
//                        up and counted (stats[4]).  Nothing spins and nothing waits.
//   voxel_match_best     a thread per slot: best_prev[b] = max over a of (C << 32 | ~a), best_cur[a] = max over b of (C << 32 | ~b), by
//                        64-bit atomicMax -- the largest C, the smallest id among equal ones, in any order of arrival; the slot's row of
//                        `pairs`; the sum of C and the number of pairs.
//   voxel_match_decide   ONE workgroup of 1024 threads, a thread per run of ceil(n_cur / 1024) neighbouring b: the match test, then an
//                        exclusive scan (wave scans and 16 partial sums in LDS) of "unmatched and has a voxel" gives every new track its
//                        rank in ascending b; cur_track, match, cur_info; then, a thread per a, prev_info and the lost rows; thread 0
//                        moves track_counter on and writes stats.
//   voxel_match_relabel  track_vol[v] = cur_track[cur[v]], track_ids[p] = cur_track[ids[p]]: a plain gather (launched only if asked for).
//
// The kernels carry no id of the optional profiler (pca_profile_enable): its tables are closed; rocprofv3 names them.
// Out of scope: motion models or prediction, re-identifying a track after a sample in which it was unmatched, merging or splitting
// instances, Hungarian or other globally optimal assignment, velocities, different px or nz between the two samples.
#include "pca_common.h"

#define MATCH_THREADS 256
#define MATCH_WAVES (MATCH_THREADS / 64)
#define MATCH_MAX_G 2048
#define MATCH_DECIDE_THREADS 1024
#define MATCH_EMPTY 0xffffffffffffffffull
#define MATCH_ACC 16              // u64 counters in the workspace: 0 cur voxels with a row, 1 in view, 2 sum C, 3 pairs, 4 dropped,
                                  // 8 cur voxels skipped, 9 prev voxels skipped (the places of `stats`)

typedef unsigned long long match_u64;

struct alignas(16) MatchArgs {
    int px, nz, G, segs;          // segs: 64-col segments of a line
    int n_prev, n_cur;
    uint32_t cap, min_overlap;
    int64_t cells, lines, n_ids, zero_words;
    double min_iou;
    double M[12];
    const int32_t *prev, *cur, *prev_track, *ids;
    int32_t *track_counter;
    // workspace
    match_u64 *keys;              // [cap], MATCH_EMPTY or a << 32 | b
    uint32_t *counts;             // [cap]; from here to the end the workspace is zeroed as `zero_words` dwords
    match_u64 *best_prev, *best_cur, *acc;
    uint32_t *vox_cur, *in_view, *vox_prev, *prev_match;
    int32_t *ws_track, *ws_match;
    // outputs
    int32_t *cur_track, *match;
    uint32_t *cur_info, *prev_info;
    int32_t *track_vol, *track_ids;
    uint32_t *pairs;
    int64_t *stats;
};

__global__ __launch_bounds__(MATCH_THREADS) void voxel_match_init(const MatchArgs a)
{
    const int64_t n = (int64_t)a.cap + a.zero_words, stride = (int64_t)a.G * MATCH_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * MATCH_THREADS + threadIdx.x; i < n; i += stride) {
        if (i < (int64_t)a.cap) a.keys[i] = MATCH_EMPTY;
        else a.counts[i - a.cap] = 0u;
    }
}

// Is this lane the head of a run of equal (ok, k0, k1) along the wave, and which lanes does its run hold?  Every lane of the wave calls.
template <bool FOLD>
__device__ __forceinline__ bool match_run_head(bool ok, uint32_t k0, uint32_t k1, int lane, match_u64 &mask)
{
    if (!FOLD) { mask = 1ull << lane; return ok; }
    const uint32_t p0 = __shfl_up(k0, 1), p1 = __shfl_up(k1, 1), pok = __shfl_up(ok ? 1u : 0u, 1);
    const bool head = lane == 0 || p0 != k0 || p1 != k1 || (pok != 0u) != ok;
    const match_u64 heads = __ballot(head);
    const match_u64 above = lane == 63 ? 0ull : heads & (~0ull << (lane + 1));
    const int next = above ? __ffsll((long long)above) - 1 : 64;
    mask = (next == 64 ? ~0ull : (1ull << next) - 1ull) & (~0ull << lane);
    return head && ok;
}

// C(a, b) += n.  At most cap probes; false: given up.
__device__ __forceinline__ bool match_insert(const MatchArgs &a, uint32_t ia, uint32_t ib, uint32_t n)
{
    const match_u64 key = ((match_u64)ia << 32) | ib;
    uint32_t h = ia * 0x9e3779b1u ^ ib * 0x85ebca6bu;
    h ^= h >> 15;
    const uint32_t mask = a.cap - 1u;
    for (uint32_t i = 0; i < a.cap; ++i) {
        const uint32_t s = (h + i) & mask;
        match_u64 k = __hip_atomic_load(a.keys + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == MATCH_EMPTY) {
            k = atomicCAS(a.keys + s, MATCH_EMPTY, key);
            if (k == MATCH_EMPTY) k = key;
        }
        if (k == key) { atomicAdd(a.counts + s, n); return true; }
    }
    return false;
}

template <bool FOLD>
__global__ __launch_bounds__(MATCH_THREADS) void voxel_match_count(const MatchArgs a)
{
    const int lane = (int)threadIdx.x & 63, px = a.px;
    const int64_t half = a.lines * a.segs, stride = (int64_t)a.G * MATCH_WAVES;
    uint32_t n_row = 0, n_view = 0, n_drop = 0, n_skip_cur = 0, n_skip_prev = 0;
    const double m00 = a.M[0], m01 = a.M[1], m02 = a.M[2], m03 = a.M[3], m10 = a.M[4], m11 = a.M[5], m12 = a.M[6], m13 = a.M[7],
                 m20 = a.M[8], m21 = a.M[9], m22 = a.M[10], m23 = a.M[11];

    for (int64_t t = (int64_t)blockIdx.x * MATCH_WAVES + ((int)threadIdx.x >> 6); t < 2 * half; t += stride) {      // (wave-uniform)
        const bool is_cur = t < half;
        const int64_t u = is_cur ? t : t - half, line = u / a.segs;
        const int col = (int)(u - line * a.segs) * 64 + lane;
        const bool on = col < px;
        int32_t id = -1;
        if (on) id = pca_ldg((is_cur ? a.cur : a.prev) + line * px + col);
        match_u64 mask;
        if (!is_cur) {
            const bool ok = id >= 0 && id < a.n_prev;
            n_skip_prev += on && !ok && id != -1;
            if (match_run_head<FOLD>(ok, ok ? (uint32_t)id : 0u, 0u, lane, mask)) atomicAdd(a.vox_prev + id, (uint32_t)__popcll(mask));
            continue;
        }
        const bool ok = id >= 0 && id < a.n_cur;
        n_skip_cur += on && !ok && id != -1;
        n_row += ok;
        const int k = (int)(line / px), row = (int)(line - (int64_t)k * px);
        bool view = false;
        int32_t ia = -1;
        if (ok) {
            const double x = (double)col + 0.5, y = (double)row + 0.5, z = (double)k + 0.5;
            const double q0 = ((m00 * x + m01 * y) + m02 * z) + m03;
            const double q1 = ((m10 * x + m11 * y) + m12 * z) + m13;
            const double q2 = ((m20 * x + m21 * y) + m22 * z) + m23;
            view = q0 >= 0.0 && q0 < (double)px && q1 >= 0.0 && q1 < (double)px && q2 >= 0.0 && q2 < (double)a.nz;
            // (in view: each floor lies in 0 .. px - 1 / nz - 1, the read is inside prev)
            if (view) ia = pca_ldg(a.prev + ((int64_t)(int)floor(q2) * px + (int)floor(q1)) * px + (int)floor(q0));
        }
        n_view += view;
        const match_u64 in_view = __ballot(view);
        if (match_run_head<FOLD>(ok, ok ? (uint32_t)id : 0u, 0u, lane, mask)) {
            atomicAdd(a.vox_cur + id, (uint32_t)__popcll(mask));
            const uint32_t c = (uint32_t)__popcll(mask & in_view);
            if (c) atomicAdd(a.in_view + id, c);
        }
        const bool pair = view && ia >= 0 && ia < a.n_prev;
        if (match_run_head<FOLD>(pair, pair ? (uint32_t)ia : 0u, pair ? (uint32_t)id : 0u, lane, mask)) {
            const uint32_t n = (uint32_t)__popcll(mask);
            if (!match_insert(a, (uint32_t)ia, (uint32_t)id, n)) n_drop += n;
        }
    }
    // (a thread's counts and a wave's sums stay below 2^32: the volume holds at most 2^25 voxels)
    const uint32_t r0 = wave_reduce_add(n_row), r1 = wave_reduce_add(n_view), r4 = wave_reduce_add(n_drop),
                   r8 = wave_reduce_add(n_skip_cur), r9 = wave_reduce_add(n_skip_prev);
    if (lane == 0) {
        if (r0) atomicAdd(a.acc + 0, (match_u64)r0);
        if (r1) atomicAdd(a.acc + 1, (match_u64)r1);
        if (r4) atomicAdd(a.acc + 4, (match_u64)r4);
        if (r8) atomicAdd(a.acc + 8, (match_u64)r8);
        if (r9) atomicAdd(a.acc + 9, (match_u64)r9);
    }
}

__global__ __launch_bounds__(MATCH_THREADS) void voxel_match_best(const MatchArgs a)
{
    const int lane = (int)threadIdx.x & 63;
    const int64_t stride = (int64_t)a.G * MATCH_THREADS;
    uint32_t sum_c = 0, n_pairs = 0;
    for (int64_t s = (int64_t)blockIdx.x * MATCH_THREADS + threadIdx.x; s < (int64_t)a.cap; s += stride) {
        const match_u64 key = pca_ldg(a.keys + s);
        uint32_t ia = 0xffffffffu, ib = 0xffffffffu, c = 0xffffffffu;
        if (key != MATCH_EMPTY) {
            ia = (uint32_t)(key >> 32); ib = (uint32_t)key; c = pca_ldg(a.counts + s);
            // (ia < n_prev and ib < n_cur: only such keys are inserted)
            atomicMax(a.best_prev + ib, ((match_u64)c << 32) | (0xffffffffu - ia));
            atomicMax(a.best_cur + ia, ((match_u64)c << 32) | (0xffffffffu - ib));
            sum_c += c; ++n_pairs;
        }
        if (a.pairs) { a.pairs[3 * s] = ia; a.pairs[3 * s + 1] = ib; a.pairs[3 * s + 2] = c; }
    }
    const uint32_t r2 = wave_reduce_add(sum_c), r3 = wave_reduce_add(n_pairs);
    if (lane == 0) {
        if (r2) atomicAdd(a.acc + 2, (match_u64)r2);
        if (r3) atomicAdd(a.acc + 3, (match_u64)r3);
    }
}

// the sum of v over the workgroup's 1024 threads; `excl`: the sum over the threads before this one
__device__ __forceinline__ uint32_t match_block_scan(uint32_t v, uint32_t *s_part, uint32_t &excl)
{
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint32_t incl = wave_incl_scan_add(v);
    __syncthreads();              // (s_part may still be read from the call before)
    if (lane == 63) s_part[w] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (int i = 0; i < MATCH_DECIDE_THREADS / 64; ++i) {
        const uint32_t p = s_part[i];
        if (i < w) before += p;
        total += p;
    }
    excl = before + incl - v;
    return total;
}

__global__ __launch_bounds__(MATCH_DECIDE_THREADS) void voxel_match_decide(const MatchArgs a)
{
    __shared__ uint32_t s_part[MATCH_DECIDE_THREADS / 64];
    const int tid = (int)threadIdx.x;
    const int32_t t0 = *a.track_counter;          // (every thread reads it here; thread 0 writes it after the last barrier)
    const int per = (a.n_cur + MATCH_DECIDE_THREADS - 1) / MATCH_DECIDE_THREADS;
    const int b0 = tid * per < a.n_cur ? tid * per : a.n_cur, b1 = b0 + per < a.n_cur ? b0 + per : a.n_cur;
    uint32_t n_new = 0, n_matched = 0;
    for (int b = b0; b < b1; ++b) {
        const uint32_t vc = a.vox_cur[b];
        const match_u64 bp = a.best_prev[b];
        int32_t m = -1;
        uint32_t c = 0, best1 = 0;
        if (bp) {
            c = (uint32_t)(bp >> 32);
            const uint32_t ia = 0xffffffffu - (uint32_t)bp;
            best1 = ia + 1u;
            const match_u64 bc = a.best_cur[ia];
            const int64_t uni = (int64_t)a.vox_prev[ia] + (int64_t)vc - (int64_t)c;
            if (0xffffffffu - (uint32_t)bc == (uint32_t)b && c >= a.min_overlap && (double)c >= a.min_iou * (double)uni) m = (int32_t)ia;
        }
        a.ws_match[b] = m;
        if (m >= 0) { a.prev_match[m] = (uint32_t)b + 1u; ++n_matched; }      // (mutual bests: one b per a)
        else if (vc) ++n_new;
        if (a.match) a.match[b] = m;
        if (a.cur_info) { uint32_t *o = a.cur_info + 4 * (int64_t)b; o[0] = vc; o[1] = a.in_view[b]; o[2] = c; o[3] = best1; }
    }
    uint32_t rank;
    const uint32_t total_new = match_block_scan(n_new, s_part, rank);
    for (int b = b0; b < b1; ++b) {
        const int32_t m = a.ws_match[b];
        int32_t track = -1;
        if (m >= 0) track = a.prev_track ? a.prev_track[m] : m;
        else if (a.vox_cur[b]) track = (int32_t)((uint32_t)t0 + rank++);
        a.ws_track[b] = track;
        if (a.cur_track) a.cur_track[b] = track;
    }
    __syncthreads();              // (prev_match, written above by other threads of this workgroup)
    uint32_t n_lost = 0;
    for (int ia = tid; ia < a.n_prev; ia += MATCH_DECIDE_THREADS) {
        const uint32_t vp = a.vox_prev[ia], pm = a.prev_match[ia];
        const match_u64 bc = a.best_cur[ia];
        n_lost += vp != 0u && pm == 0u;
        if (a.prev_info) {
            uint32_t *o = a.prev_info + 4 * (int64_t)ia;
            o[0] = vp; o[1] = (uint32_t)(bc >> 32); o[2] = bc ? 0xffffffffu - (uint32_t)bc + 1u : 0u; o[3] = pm;
        }
    }
    uint32_t unused;
    const uint32_t total_matched = match_block_scan(n_matched, s_part, unused);
    const uint32_t total_lost = match_block_scan(n_lost, s_part, unused);
    if (tid == 0) {
        *a.track_counter = (int32_t)((uint32_t)t0 + total_new);
        if (a.stats) {
            for (int i = 0; i < 10; ++i) a.stats[i] = (int64_t)a.acc[i];
            a.stats[5] = total_matched; a.stats[6] = total_new; a.stats[7] = total_lost;
        }
    }
}

__global__ __launch_bounds__(MATCH_THREADS) void voxel_match_relabel(const MatchArgs a)
{
    const int64_t n_vol = a.track_vol ? a.cells : 0, n = n_vol + (a.track_ids ? a.n_ids : 0), stride = (int64_t)a.G * MATCH_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * MATCH_THREADS + threadIdx.x; i < n; i += stride) {
        const bool vol = i < n_vol;
        const int32_t id = pca_ldg(vol ? a.cur + i : a.ids + (i - n_vol));
        const int32_t t = id >= 0 && id < a.n_cur ? pca_ldg(a.ws_track + id) : -1;
        if (vol) a.track_vol[i] = t; else a.track_ids[i - n_vol] = t;
    }
}

static bool match_shape_ok(int n_prev, int n_cur, int cap_pairs)
{
    return n_prev >= 1 && n_prev <= 65536 && n_cur >= 1 && n_cur <= 65536 && cap_pairs >= 16 && cap_pairs <= (1 << 22) &&
           (cap_pairs & (cap_pairs - 1)) == 0;
}

extern "C" {

int64_t pca_voxel_instance_match_workspace_bytes(int n_prev, int n_cur, int cap_pairs)
{
    if (!match_shape_ok(n_prev, n_cur, cap_pairs)) return -1;
    return pca_align256((int64_t)cap_pairs * 8) + pca_align256((int64_t)cap_pairs * 4) + pca_align256((int64_t)n_cur * 8) +
           pca_align256((int64_t)n_prev * 8) + pca_align256(MATCH_ACC * 8) + 4 * pca_align256((int64_t)n_cur * 4) +
           2 * pca_align256((int64_t)n_prev * 4);
}

int pca_voxel_instance_match(pca_ctx *ctx, int px, int nz, const int32_t *prev, int n_prev, const int32_t *cur, int n_cur,
                             const double *M, int min_overlap, double min_iou, int cap_pairs, const int32_t *prev_track,
                             int32_t *track_counter, const int32_t *ids, int64_t n_ids, void *workspace, int64_t workspace_bytes,
                             int32_t *cur_track, int32_t *match, uint32_t *cur_info, uint32_t *prev_info, int32_t *track_vol,
                             int32_t *track_ids, uint32_t *pairs, int64_t *stats, void *stream)
{
    if (!ctx) return -1;
    hipStream_t s = (hipStream_t)stream;
    const std::string w("voxel instance match");
    // every check comes before the first launch
    if (px < 1 || px > 1024) { ctx->err = w + ": px must be in 1..1024"; return -1; }
    if (nz < 1 || nz > 32) { ctx->err = w + ": nz must be in 1..32"; return -1; }
    if (n_prev < 1 || n_prev > 65536 || n_cur < 1 || n_cur > 65536) { ctx->err = w + ": n_prev and n_cur must be in 1..65536"; return -1; }
    if (!prev || !cur) { ctx->err = w + ": prev and cur must not be NULL"; return -1; }
    if (!M) { ctx->err = w + ": M must not be NULL"; return -1; }
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(M[i])) { ctx->err = w + ": every entry of M must be finite"; return -1; }
    if (min_overlap < 1) { ctx->err = w + ": min_overlap must be >= 1"; return -1; }
    if (!(std::isfinite(min_iou) && min_iou >= 0.0 && min_iou <= 1.0)) { ctx->err = w + ": min_iou must be finite and in 0..1"; return -1; }
    if (cap_pairs < 16 || cap_pairs > (1 << 22) || (cap_pairs & (cap_pairs - 1))) {
        ctx->err = w + ": cap_pairs must be a power of two in 16..2^22"; return -1;
    }
    if (!track_counter) { ctx->err = w + ": track_counter must not be NULL"; return -1; }
    if (n_ids < 0 || (n_ids > 0 && !ids)) { ctx->err = w + ": ids must hold n_ids >= 0 entries"; return -1; }
    if (track_ids && !ids) { ctx->err = w + ": track_ids needs ids"; return -1; }
    if (!cur_track && !match && !cur_info && !prev_info && !track_vol && !track_ids && !pairs && !stats) {
        ctx->err = w + ": at least one output is needed"; return -1;
    }
    const int64_t need = pca_voxel_instance_match_workspace_bytes(n_prev, n_cur, cap_pairs);
    if (!workspace || workspace_bytes < need) {
        ctx->err = w + ": workspace too small (pca_voxel_instance_match_workspace_bytes)"; return -1;
    }
    if ((uintptr_t)workspace & 7) { ctx->err = w + ": workspace must be 8-byte aligned"; return -1; }

    MatchArgs A;
    A.px = px; A.nz = nz; A.segs = (px + 63) / 64;
    A.n_prev = n_prev; A.n_cur = n_cur;
    A.cap = (uint32_t)cap_pairs; A.min_overlap = (uint32_t)min_overlap;
    A.cells = (int64_t)nz * px * px; A.lines = (int64_t)nz * px; A.n_ids = track_ids ? n_ids : 0;
    A.min_iou = min_iou;
    for (int i = 0; i < 12; ++i) A.M[i] = M[i];
    A.prev = prev; A.cur = cur; A.prev_track = prev_track; A.ids = ids; A.track_counter = track_counter;
    {
        uint8_t *p = reinterpret_cast<uint8_t *>(workspace);
        auto take = [&p](int64_t bytes) { uint8_t *r = p; p += pca_align256(bytes); return r; };
        A.keys = reinterpret_cast<match_u64 *>(take((int64_t)cap_pairs * 8));
        A.counts = reinterpret_cast<uint32_t *>(take((int64_t)cap_pairs * 4));
        A.best_prev = reinterpret_cast<match_u64 *>(take((int64_t)n_cur * 8));
        A.best_cur = reinterpret_cast<match_u64 *>(take((int64_t)n_prev * 8));
        A.acc = reinterpret_cast<match_u64 *>(take(MATCH_ACC * 8));
        A.vox_cur = reinterpret_cast<uint32_t *>(take((int64_t)n_cur * 4));
        A.in_view = reinterpret_cast<uint32_t *>(take((int64_t)n_cur * 4));
        A.ws_track = reinterpret_cast<int32_t *>(take((int64_t)n_cur * 4));
        A.ws_match = reinterpret_cast<int32_t *>(take((int64_t)n_cur * 4));
        A.vox_prev = reinterpret_cast<uint32_t *>(take((int64_t)n_prev * 4));
        A.prev_match = reinterpret_cast<uint32_t *>(take((int64_t)n_prev * 4));
        A.zero_words = (p - reinterpret_cast<uint8_t *>(A.counts)) / 4;             // (p - workspace == need)
    }
    A.cur_track = cur_track; A.match = match; A.cur_info = cur_info; A.prev_info = prev_info;
    A.track_vol = track_vol; A.track_ids = track_ids; A.pairs = pairs; A.stats = stats;
    // PCA_VOXEL_MATCH_G: a cap on the workgroups of every kernel but the one-workgroup decide, read on every call (tests send one
    // workgroup round its loops); PCA_VOXEL_MATCH_FOLD=0: every voxel makes its own atomics (the A/B of profiles/voxel_instance_match.txt)
    const int64_t max_g = pca_env_int("PCA_VOXEL_MATCH_G", MATCH_MAX_G, 1, MATCH_MAX_G);
    const bool fold = pca_env_int("PCA_VOXEL_MATCH_FOLD", 1, 0, 1) != 0;
    auto groups = [max_g](int64_t items, int per) { const int64_t g = (items + per - 1) / per; return (int)(g < 1 ? 1 : (g < max_g ? g : max_g)); };
    PCA_CHECK(ctx, hipSetDevice(ctx->device));
    const MatchArgs &args = A;
    A.G = groups((int64_t)A.cap + A.zero_words, MATCH_THREADS);
    hipLaunchKernelGGL(voxel_match_init, dim3(args.G), dim3(MATCH_THREADS), 0, s, args);
    A.G = groups(2 * A.lines * A.segs, MATCH_WAVES);
    if (fold) hipLaunchKernelGGL(voxel_match_count<true>, dim3(args.G), dim3(MATCH_THREADS), 0, s, args);
    else hipLaunchKernelGGL(voxel_match_count<false>, dim3(args.G), dim3(MATCH_THREADS), 0, s, args);
    A.G = groups(A.cap, MATCH_THREADS);
    hipLaunchKernelGGL(voxel_match_best, dim3(args.G), dim3(MATCH_THREADS), 0, s, args);
    A.G = 1;
    hipLaunchKernelGGL(voxel_match_decide, dim3(1), dim3(MATCH_DECIDE_THREADS), 0, s, args);
    if (track_vol || track_ids) {
        A.G = groups((track_vol ? A.cells : 0) + A.n_ids, MATCH_THREADS);
        hipLaunchKernelGGL(voxel_match_relabel, dim3(args.G), dim3(MATCH_THREADS), 0, s, args);
    }
    PCA_CHECK(ctx, hipGetLastError());
    return 0;
}

}  // extern "C"
