// pca_point_pass.h -- what the read-only passes that visit the window one stored point per thread share (bev_voxel_rays; bev_carve_ends,
// bev_carve_rays, bev_carve_flags; render_zbuffer, render_resolve; bev_inst_points; bev_box_count, bev_box_scatter), as pca_bev_side.h is what the tiled passes
// share: the window and its cuts, the slot of a point, the counters' way to memory and the host's launch size.  The ONE copy of
// each; the next pass of this family starts here.  Args: any argument block with st, frame_off, slot_begin, slot_end and
// max_points (RayArgs, CarveArgs, RenderArgs; InstArgs hands in its v.s) -- no common base: every block keeps its own offsets.
#pragma once
#include "pca_bev_view.h"

#define POINT_THREADS 256         // threads of a workgroup = points of a chunk
#define POINT_MAX_G 2048          // workgroups at most of a kernel that strides over the chunks (eight per CU)

// The window's points [lo, hi): cut at max_points, then at the capacity (nothing is stored behind it, whatever frame_off
// counts).  Only the max_points cut is an overflow; RAISE: thread 0 of workgroup 0 reports it through a.status (the first kernel
// of a pass).
struct PointWindow { int64_t lo, hi; };
template <bool RAISE, typename Args>
__device__ __forceinline__ PointWindow point_window(const Args &a)
{
    PointWindow w;
    w.lo = pca_sload(a.frame_off + a.slot_begin);
    const int64_t hi0 = pca_sload(a.frame_off + a.slot_end);
    const bool cut = hi0 - w.lo > a.max_points;
    w.hi = cut ? w.lo + a.max_points : hi0;
    if (w.hi > a.st.capacity) w.hi = a.st.capacity;
    if constexpr (RAISE)
        if (cut && blockIdx.x == 0 && threadIdx.x == 0) pca_raise(a.status, PCA_STATUS_STORE_OVERFLOW);
    return w;
}
// the slot of a chunk's first point: the last one with frame_off[slot] <= c_lo (scalar loads: the chunk is workgroup-uniform)
template <typename Args>
__device__ __forceinline__ int point_chunk_slot(const Args &a, int64_t c_lo)
{
    int s_lo = a.slot_begin, s_hi = a.slot_end;
    while (s_hi - s_lo > 1) {
        const int mid = (s_lo + s_hi) >> 1;
        if (pca_sload(a.frame_off + mid) <= c_lo) s_lo = mid; else s_hi = mid;
    }
    return s_lo;
}
// the slot of the lane's own point p of that chunk (p < hi <= frame_off[slot_end]: the walk ends below slot_end; empty frames
// are stepped over)
template <typename Args>
__device__ __forceinline__ int point_lane_slot(const Args &a, int s_lo, int64_t p)
{
    int slot = s_lo;
    while (slot + 1 < a.slot_end && pca_ldg(a.frame_off + slot + 1) <= p) ++slot;
    return slot;
}
// The counters of a workgroup, n... per lane (uint32_t each): wave, LDS, one global add per counter at dst + k, skipped where
// zero (dst may be null).  Every thread calls it, outside divergent code.  The LDS words belong to the instantiation; a kernel
// may call the same one twice (bev_inst_points does): word k is cleared by the thread that read it.
template <typename... U>
__device__ __forceinline__ void point_count(unsigned long long *dst, U... n)
{
    constexpr int N = (int)sizeof...(U);
    __shared__ unsigned long long s_sum[N];
    const uint32_t lane_n[N] = {n...};
    const int tid = (int)threadIdx.x;
    if (tid < N) s_sum[tid] = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const uint32_t w = wave_reduce_add(lane_n[k]);
        if ((tid & 63) == 0) atomicAdd(&s_sum[k], (unsigned long long)w);
    }
    __syncthreads();
    if (tid < N && dst && s_sum[tid]) atomicAdd(dst + tid, s_sum[tid]);
}

// ---- aggregation in front of a few hot keys (bev_inst_compress, bev_inst_write, bev_inst_points; bev_box_count, bev_box_scatter) ----
// Every lane calls it with its key (0xffffffff: none).  f(key, lanes, leader) runs once per DISTINCT key of the wave, on all
// lanes (it may reduce over the wave): `lanes` = the ballot of the lanes that hold the key, `leader` = this lane is their first.
template <typename F>
__device__ __forceinline__ void inst_for_each_key(uint32_t key, F f)
{
    unsigned long long todo = __ballot(key != 0xffffffffu);
    while (todo) {                                          // (bounded by the wave's distinct keys, 64 at most)
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t kk = (uint32_t)__builtin_amdgcn_readlane((int)key, leader);
        const unsigned long long same = __ballot(key == kk);
        f(kk, same, (int)(threadIdx.x & 63) == leader);
        todo &= ~same;
    }
}
// A workgroup's direct-mapped LDS cache in front of the global atomics on a few hot rows: a key claims its slot by
// compare-and-swap; a key whose slot another key holds goes to global memory directly (claim returns -1).  The sums (val[0]) or
// the six extremes (min, max, min, max, min, max) of a slot are flushed by the kernel's last lines, one global atomic each.
#define INST_SLOTS 64
struct InstSlots { uint32_t key[INST_SLOTS]; uint32_t val[INST_SLOTS][6]; };
__device__ __forceinline__ void inst_slots_init(InstSlots &s, bool extremes)
{
    if (threadIdx.x < INST_SLOTS) {
        s.key[threadIdx.x] = 0xffffffffu;
        for (int j = 0; j < 6; ++j) s.val[threadIdx.x][j] = extremes && !(j & 1) ? 0xffffffffu : 0u;
    }
    __syncthreads();
}
__device__ __forceinline__ int inst_slots_claim(InstSlots &s, uint32_t key)
{
    const int slot = (int)((key * 2654435761u) >> 26);
    const uint32_t old = atomicCAS(&s.key[slot], 0xffffffffu, key);
    return old == 0xffffffffu || old == key ? slot : -1;
}

// ---- host side ----
static inline int64_t point_chunks(int64_t max_points) { return (max_points + POINT_THREADS - 1) / POINT_THREADS; }
// workgroups of a kernel that strides over the chunks of max_points items; env (PCA_*_G): a cap on them, read on every call (tests
// set it to send a workgroup round its loop again)
static inline int point_pass_G(int64_t max_points, const char *env)
{
    const int64_t chunks = point_chunks(max_points), max_g = pca_env_int(env, POINT_MAX_G, 1, POINT_MAX_G);
    return (int)(chunks > max_g ? max_g : chunks);
}
