// pca_bev_carve.hip -- free-space carving by ray hit / miss: the counting form of the rays of pca_bev_rays.hip.  A voxel that held
// points of a movable class at one moment, and that the beams of other frames later passed straight through, held a moving
// object: its points are flagged, and DeviceStore.bev_voxel_carve(mark_dyn=True) writes dyn = 1 for them.  The geometry, the
// drop rules, the traversal and its tie order are those of bev_voxel_rays, from the one copy in pca_bev_ray_setup.h.
//
//   bev_carve_ends   one thread per stored point of the window, 256 threads, a grid-stride loop over chunks of 256 points with
//                    the window and the chunk / slot walk of pca_point_pass.h.  The end voxel of the point's ray: vox[p] = its place in the
//                    output, or -1 (the point takes no part, its ray is dropped, or it ends outside the grid); a no-return
//                    u32 atomic add on hits; a byte store of 1 into cand for a point of a class in `only` (every writer writes
//                    the same value).  Counters 0..3 per lane, then point_count (pca_point_pass.h).
//   bev_carve_rays   the traversal, stopped end_margin steps before the end voxel.  Per step inside the grid a byte load of
//                    cand (u8 [nz][px][px], 2 MiB at 256^2 x 32: it stays in L2) and, only where that reads 1, a no-return
//                    u32 atomic add on cross: global atomics execute at the memory side, and scattered ones run far below
//                    the rate of plain stores, while candidate voxels are a small part of the steps on real data.  Hence
//                    cross is 0 for every voxel that is not a candidate voxel: part of the contract.  The byte is looked at
//                    one step later, beside the next step's arithmetic, as bev_voxel_rays looks at its mark.  A ray leaves its
//                    loop early only by integer tests that cannot change the counted set.
//   bev_carve_flags  one thread per point: vox, class, hits, cross -> the flag byte; counters 4 and 5.
// Scope: ONE origin per stored frame; the rays of a point's own frame count like any other -- end_margin is what keeps a
// surface from carving itself (the neighbouring beams of one surface cross its own voxels just before they end); nothing calls
// this from integrate().  All sums are integer sums: the result does not depend on the order.  The store is never written.
#include "pca_bev_ray_setup.h"
#include "pca_point_pass.h"

struct alignas(16) CarveArgs {
    pca_store st;
    const int64_t *frame_off;
    int slot_begin, slot_end;
    int64_t max_points;
    pca_bev_params prm;
    BevOwed owed;                 // owed re-transforms: applied to the points that are read, never written back
    double z_lo, z_step;
    int nz, include_dyn;
    int G;                        // workgroups of bev_carve_ends and bev_carve_rays
    int end_margin;
    uint32_t min_cross;
    double ratio;
    ClassMask only;               // the classes that may be flagged
    const double *origins;        // [slot_end - slot_begin][3]: the sensor position of each slot (nothing owed)
    int32_t *vox;                 // [max_points], by window index: the end voxel's place in the output, or -1
    uint8_t *cand;                // [nz][px][px]: 1 = a candidate voxel
    uint32_t *hits, *cross;       // [nz][px][px]
    uint8_t *flags;               // [window points] or NULL
    unsigned long long *stats;    // [6] or NULL
    uint32_t *status;             // context status word (PCA_STATUS_* bits)
};

// The ray of point p (which takes part): start and end in grid coordinates.  Returns whether all six are usable.
__device__ __forceinline__ bool carve_ray(const CarveArgs &a, const RayGrid &q, const PendHi &pend_hi, int64_t p, int s_lo,
                                          double &s0, double &s1, double &s2, double &e0, double &e1, double &e2)
{
    const int slot = point_lane_slot(a, s_lo, p);
    double X = pca_ldg(a.st.x + p), Y = pca_ldg(a.st.y + p), Z = pca_ldg(a.st.z + p);
    apply_owed(a.owed, pend_hi, p, X, Y, Z);
    const double *o = a.origins + (int64_t)(slot - a.slot_begin) * 3;
    ray_coords(q, pca_ldg(o), pca_ldg(o + 1), pca_ldg(o + 2), s0, s1, s2);
    ray_coords(q, X, Y, Z, e0, e1, e2);
    return ray_coord_ok(s0) && ray_coord_ok(s1) && ray_coord_ok(s2) && ray_coord_ok(e0) && ray_coord_ok(e1) && ray_coord_ok(e2);
}

__global__ __launch_bounds__(POINT_THREADS) void bev_carve_ends(const CarveArgs a)
{
    const int tid = (int)threadIdx.x;
    const PointWindow w = point_window<true>(a);
    const int64_t lo = w.lo, hi = w.hi;
    const PendHi pend_hi = owed_bounds(a.owed, a.frame_off, a.slot_begin, lo);
    const RayGrid q = ray_grid(a.prm, a.z_lo, a.z_step);
    const int px = a.prm.px, nz = a.nz;
    uint32_t n_part = 0, n_cast = 0, n_not_finite = 0, n_too_long = 0;

    for (int64_t c_lo = lo + (int64_t)blockIdx.x * POINT_THREADS; c_lo < hi; c_lo += (int64_t)a.G * POINT_THREADS) {
        const int s_lo = point_chunk_slot(a, c_lo);
        const int64_t p = c_lo + tid;
        if (p >= hi) continue;
        int32_t place = -1;
        if (a.include_dyn || pca_ldg(a.st.dyn + p) != 1) {
            ++n_part;
            double s0, s1, s2, e0, e1, e2;
            if (!carve_ray(a, q, pend_hi, p, s_lo, s0, s1, s2, e0, e1, e2)) {
                ++n_not_finite;
            } else {
                const RayVoxels r = ray_voxels(s0, s1, s2, e0, e1, e2);
                if (ray_steps(r) > PCA_BEV_RAYS_MAX_STEPS) {
                    ++n_too_long;
                } else {
                    ++n_cast;
                    if ((unsigned)r.g0 < (unsigned)px && (unsigned)r.g1 < (unsigned)px && (unsigned)r.g2 < (unsigned)nz) {
                        place = (r.g2 * px + (px - 1 - r.g1)) * px + r.g0;          // (< 2^25: px <= 1024, nz <= 32)
                        atomicAdd(a.hits + place, 1u);
                        if (in_mask(a.only, pca_ldg(a.st.rgbs + p) >> 24)) a.cand[place] = 1;
                    }
                }
            }
        }
        a.vox[p - lo] = place;
    }
    point_count(a.stats, n_part, n_cast, n_not_finite, n_too_long);
}

__global__ __launch_bounds__(POINT_THREADS) void bev_carve_rays(const CarveArgs a)
{
    const int tid = (int)threadIdx.x;
    const PointWindow w = point_window<false>(a);
    const int64_t lo = w.lo, hi = w.hi;
    const PendHi pend_hi = owed_bounds(a.owed, a.frame_off, a.slot_begin, lo);
    const RayGrid q = ray_grid(a.prm, a.z_lo, a.z_step);
    const int px = a.prm.px, nz = a.nz;
    auto *cand = reinterpret_cast<const __attribute__((address_space(1))) uint8_t *>(reinterpret_cast<uintptr_t>(a.cand));

    for (int64_t c_lo = lo + (int64_t)blockIdx.x * POINT_THREADS; c_lo < hi; c_lo += (int64_t)a.G * POINT_THREADS) {
        const int s_lo = point_chunk_slot(a, c_lo);
        const int64_t p = c_lo + tid;
        if (p >= hi) continue;
        if (!a.include_dyn && pca_ldg(a.st.dyn + p) == 1) continue;
        double s0, s1, s2, e0, e1, e2;
        if (!carve_ray(a, q, pend_hi, p, s_lo, s0, s1, s2, e0, e1, e2)) continue;
        RayVoxels r = ray_voxels(s0, s1, s2, e0, e1, e2);
        const int64_t N64 = ray_steps(r);
        if (N64 > PCA_BEV_RAYS_MAX_STEPS) continue;
        const int M = (int)N64 - a.end_margin;              // the steps that count: it < N - end_margin
        // integer early exit 1: nothing counts, or the ray's voxel bounding box misses the grid
        if (M <= 0 || ray_box_misses(r, px, nz)) continue;
        RayMarch m = ray_march(r, s0, s1, s2, e0, e1, e2);
        // a step's byte is looked at one step later (pi, pv: the place of the step before and what the load gave), so that the
        // load's round trip runs beside a whole step's arithmetic
        uint32_t pi = 0;
        uint8_t pv = 0;
        for (int it = 0; it < M; ++it) {
            uint32_t i = 0;
            uint8_t v = 0;
            if ((unsigned)r.c0 < (unsigned)px && (unsigned)r.c1 < (unsigned)px && (unsigned)r.c2 < (unsigned)nz) {
                i = (uint32_t)((r.c2 * px + (px - 1 - r.c1)) * px + r.c0);
                v = cand[i];
            } else if (ray_gone(r, m, px, nz)) {
                break;                                      // integer early exit 2: outside on an axis and moving away, or not moving
            }
            if (pv == 1) atomicAdd(a.cross + pi, 1u);
            pi = i; pv = v;
            ray_advance(r, m);
        }
        if (pv == 1) atomicAdd(a.cross + pi, 1u);
    }
}

__global__ __launch_bounds__(POINT_THREADS) void bev_carve_flags(const CarveArgs a)
{
    const PointWindow w = point_window<false>(a);
    const int64_t lo = w.lo, hi = w.hi;
    const int64_t p = lo + (int64_t)blockIdx.x * POINT_THREADS + threadIdx.x;
    uint32_t n_cand = 0, n_flagged = 0;
    if (p < hi) {
        uint8_t flag = 255;
        const int32_t place = pca_ldg(a.vox + (p - lo));
        if (place >= 0 && in_mask(a.only, pca_ldg(a.st.rgbs + p) >> 24)) {
            const uint32_t h = pca_ldg(a.hits + place), c = pca_ldg(a.cross + place);
            flag = (c >= a.min_cross && (double)c >= a.ratio * (double)h) ? 1 : 0;
            ++n_cand;
            n_flagged += flag;
        }
        if (a.flags) a.flags[p - lo] = flag;
    }
    point_count(a.stats ? a.stats + 4 : nullptr, n_cand, n_flagged);
}

static const WindowPass CARVE_PASS = {"bev voxel carve", true, false};

// the workspace: vox, then cand, hits and cross, each at a 256-byte boundary
struct CarveLayout { size_t vox, cand, hits, cross, total; };
static inline CarveLayout carve_layout(int64_t max_points, int px, int nz)
{
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t cells = (size_t)(nz < 1 ? 1 : nz) * (size_t)(px < 1 ? 1 : px) * (size_t)(px < 1 ? 1 : px);
    CarveLayout l;
    l.vox = 0;
    l.cand = up((size_t)(max_points < 1 ? 1 : max_points) * sizeof(int32_t));
    l.hits = l.cand + up(cells);
    l.cross = l.hits + up(cells * sizeof(uint32_t));
    l.total = l.cross + up(cells * sizeof(uint32_t)) + 256;     // (+ 256: the base is aligned up)
    return l;
}

extern "C" {

int64_t pca_bev_carve_workspace_bytes(int64_t max_points, int px, int nz)
{
    return (int64_t)carve_layout(max_points, px, nz).total;
}

int pca_bev_voxel_carve(pca_ctx *ctx, const pca_store *store, const int64_t *frame_off, int slot_begin, int slot_end,
                        int64_t max_points, const pca_bev_params *prm, double z_lo, double z_step, int nz, int include_dyn,
                        const double *origins, const pca_class_group *only, int end_margin, uint32_t min_cross, double ratio,
                        const double *pending_Ts, const int *pending_slot_ends, int n_pending, void *workspace,
                        int64_t workspace_bytes, uint32_t *hits, uint32_t *cross, uint8_t *flags, int64_t *stats, void *stream)
{
    if (!ctx) return -1;
    if (max_points < 1) max_points = 1;
    hipStream_t s = (hipStream_t)stream;
    // every check comes before the first launch (a noted K1 and the clearing of the outputs included)
    CarveArgs A;
    if (window_check(ctx, CARVE_PASS, origins && only && workspace && (hits || cross || flags || stats), store, frame_off, slot_begin,
                     slot_begin, slot_end, max_points, prm, pending_Ts, pending_slot_ends, n_pending, A))
        return -1;
    if (voxel_grid_check(ctx, CARVE_PASS.what, z_lo, z_step, nz)) return -1;
    const std::string w(CARVE_PASS.what);
    if (end_margin < 0 || end_margin > PCA_BEV_RAYS_MAX_STEPS) { ctx->err = w + ": end_margin must be in 0..16384"; return -1; }
    if (min_cross < 1) { ctx->err = w + ": min_cross must be >= 1"; return -1; }
    if (!(ratio >= 0.0 && ratio < __builtin_huge_val())) { ctx->err = w + ": ratio must be finite and >= 0"; return -1; }
    if (max_points >= (1ll << 32)) { ctx->err = w + ": max_points must be below 2^32 (the window index is 32 bits wide)"; return -1; }
    const CarveLayout l = carve_layout(max_points, prm->px, nz);
    if (workspace_bytes < (int64_t)l.total) { ctx->err = w + ": workspace too small"; return -1; }
    char *base = reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
    A.z_lo = z_lo; A.z_step = z_step;
    A.nz = nz; A.include_dyn = include_dyn;
    A.G = point_pass_G(max_points, "PCA_BEV_CARVE_G");
    A.end_margin = end_margin; A.min_cross = min_cross; A.ratio = ratio;
    for (int i = 0; i < 4; ++i) A.only.w[i] = only->mask[i];
    A.origins = origins;
    A.vox = reinterpret_cast<int32_t *>(base + l.vox);
    A.cand = reinterpret_cast<uint8_t *>(base + l.cand);
    A.hits = hits ? hits : reinterpret_cast<uint32_t *>(base + l.hits);
    A.cross = cross ? cross : reinterpret_cast<uint32_t *>(base + l.cross);
    A.flags = flags;
    A.stats = reinterpret_cast<unsigned long long *>(stats);
    const size_t cells = (size_t)nz * prm->px * prm->px;
    PCA_CHECK(ctx, hipSetDevice(ctx->device));
    if (pca_k1_flush_pending(ctx)) return -1;               // a noted K1 runs on its own first, as before the rays
    PCA_CHECK(ctx, hipMemsetAsync(A.cand, 0, cells, s));
    PCA_CHECK(ctx, hipMemsetAsync(A.hits, 0, cells * sizeof(uint32_t), s));
    PCA_CHECK(ctx, hipMemsetAsync(A.cross, 0, cells * sizeof(uint32_t), s));
    if (stats) PCA_CHECK(ctx, hipMemsetAsync(stats, 0, 6 * sizeof(int64_t), s));
    const CarveArgs &args = A;
    if (slot_end > slot_begin)                              // (a window without a slot: no launch over zero points)
    {
        PCA_LAUNCH(ctx, PCA_K_BEV_CARVE_ENDS, bev_carve_ends, dim3(args.G), dim3(POINT_THREADS), s, args);
        PCA_LAUNCH(ctx, PCA_K_BEV_CARVE_RAYS, bev_carve_rays, dim3(args.G), dim3(POINT_THREADS), s, args);
        if (flags || stats)
            PCA_LAUNCH(ctx, PCA_K_BEV_CARVE_FLAGS, bev_carve_flags, dim3((unsigned)point_chunks(max_points)), dim3(POINT_THREADS), s, args);
    }
    PCA_CHECK(ctx, hipGetLastError());
    return 0;
}

}  // extern "C"
