// pca_bev_rays.hip -- lidar rays cast through the voxel grid of the occupancy labels (pca_bev_voxel.hip): which voxels a beam
// crossed on its way from the sensor to a stored point.  With the labels' counts this tells an empty voxel apart into free
// (a beam passed) and unseen (none did) -- the "invalid" mask of SemanticKITTI-SSC / SSCBench-KITTI-360 ground truth.
//
//   bev_voxel_rays   one thread per stored point of the window, 256 threads, a grid-stride loop over chunks of 256 points.
//                    The window, the slot of a chunk's first point and a lane's own slot are those of pca_point_pass.h (a
//                    binary search over frame_off in scalar loads, then a walk per lane); the slot's sensor position and the
//                    point (owed re-transforms applied: pca_bev_view.h) into grid coordinates -- f64, nothing fused, the
//                    IEEE divisions, the UNFUSED product sum (unlike the view test: a numpy model restates it bit for bit);
//                    Amanatides-Woo driven by the integer step counts, so that it always ends in the end voxel, which is
//                    not marked.  A mark is a byte load and, where that reads 0, a byte store of 1 into the u8 volume
//                    [nz][px][px] (2 MiB at 256^2 x 32: it stays in L2): every writer writes the same value, so no atomic
//                    is needed and the result does not depend on the order; a stale 0 from another CU's store costs one
//                    redundant store.  The byte is looked at one step later, beside the next step's arithmetic (1.56 ms
//                    against 1.62 on the headline window; ALWAYS_STORE, every mark a store without the load: 1.69 ms --
//                    profiles/bev_voxel_rays.txt).  A ray leaves its loop early only by integer tests that cannot change
//                    the marked set.  The four counters: per lane, per wave, LDS, one global add per counter and workgroup.
// The store is never written.  PCA_BEV_RAYS_MAX_STEPS bounds every ray, hence every launch.  The grid coordinates and the
// ray's set-up (voxels, step counts, tMax, tDelta) come from pca_bev_ray_setup.h, shared with pca_bev_carve.hip.  The step
// loop and the counters' epilogue stay written out here, as they were tuned: the kernel sits at 100 scalar registers, and with
// ray_box_misses / ray_gone / ray_advance or with point_count (pca_point_pass.h) in their place the step loop gains 9 to 17
// v_readlane of spilled scalars: 1.625 and 1.627 ms against 1.554-1.559 (profiles/point_pass_refactor_ab.txt).
#include "pca_bev_ray_setup.h"
#include "pca_point_pass.h"

struct alignas(16) RayArgs {
    pca_store st;
    const int64_t *frame_off;
    int slot_begin, slot_end;
    int64_t max_points;
    pca_bev_params prm;
    BevOwed owed;                 // owed re-transforms: applied to the points that are read, never written back
    double z_lo, z_step;
    int nz, include_dyn;
    int G;                        // workgroups of the launch
    const double *origins;        // [slot_end - slot_begin][3]: the sensor position of each slot (nothing owed)
    uint8_t *seen;                // [nz][px][px] or NULL
    unsigned long long *stats;    // [4] or NULL
    uint32_t *status;             // context status word (PCA_STATUS_* bits)
};

template <bool ALWAYS_STORE>
__global__ __launch_bounds__(POINT_THREADS) void bev_voxel_rays(const RayArgs a)
{
    __shared__ unsigned long long s_stat[4];
    const int tid = (int)threadIdx.x;
    if (tid < 4) s_stat[tid] = 0;
    __syncthreads();
    const PointWindow w = point_window<true>(a);
    const int64_t lo = w.lo, hi = w.hi;
    const PendHi pend_hi = owed_bounds(a.owed, a.frame_off, a.slot_begin, lo);
    const RayGrid q = ray_grid(a.prm, a.z_lo, a.z_step);
    const int px = a.prm.px, nz = a.nz;
    auto *seen = reinterpret_cast<__attribute__((address_space(1))) uint8_t *>(reinterpret_cast<uintptr_t>(a.seen));
    const double INF = __builtin_huge_val();
    uint32_t n_considered = 0, n_cast = 0, n_not_finite = 0, n_too_long = 0;

    for (int64_t c_lo = lo + (int64_t)blockIdx.x * POINT_THREADS; c_lo < hi; c_lo += (int64_t)a.G * POINT_THREADS) {
        const int s_lo = point_chunk_slot(a, c_lo);
        const int64_t p = c_lo + tid;
        if (p >= hi) continue;
        const int slot = point_lane_slot(a, s_lo, p);
        if (!a.include_dyn && pca_ldg(a.st.dyn + p) == 1) continue;
        ++n_considered;
        double X = pca_ldg(a.st.x + p), Y = pca_ldg(a.st.y + p), Z = pca_ldg(a.st.z + p);
        apply_owed(a.owed, pend_hi, p, X, Y, Z);
        const double *o = a.origins + (int64_t)(slot - a.slot_begin) * 3;
        double s0, s1, s2, e0, e1, e2;
        ray_coords(q, pca_ldg(o), pca_ldg(o + 1), pca_ldg(o + 2), s0, s1, s2);
        ray_coords(q, X, Y, Z, e0, e1, e2);
        if (!(ray_coord_ok(s0) && ray_coord_ok(s1) && ray_coord_ok(s2) && ray_coord_ok(e0) && ray_coord_ok(e1) && ray_coord_ok(e2))) {
            ++n_not_finite;
            continue;
        }
        const RayVoxels r = ray_voxels(s0, s1, s2, e0, e1, e2);
        int c0 = r.c0, c1 = r.c1, c2 = r.c2, n0 = r.n0, n1 = r.n1, n2 = r.n2;
        const int g0 = r.g0, g1 = r.g1, g2 = r.g2;
        const int64_t N64 = ray_steps(r);
        if (N64 > PCA_BEV_RAYS_MAX_STEPS) {
            ++n_too_long;
            continue;
        }
        ++n_cast;
        // integer early exit 1: the ray's voxel bounding box misses the grid (or there is nothing to mark in)
        if (!a.seen || (c0 < 0 && g0 < 0) || (c0 >= px && g0 >= px) || (c1 < 0 && g1 < 0) || (c1 >= px && g1 >= px) ||
            (c2 < 0 && g2 < 0) || (c2 >= nz && g2 >= nz))
            continue;
        const RayMarch m0 = ray_march(r, s0, s1, s2, e0, e1, e2);
        const int st0 = m0.st0, st1 = m0.st1, st2 = m0.st2;
        const double dl0 = m0.dl0, dl1 = m0.dl1, dl2 = m0.dl2;
        double t0 = m0.t0, t1 = m0.t1, t2 = m0.t2;
        const int N = (int)N64;
        // a mark's byte is looked at one step later (pm, pv: the byte of the step before and what the load gave), so that the
        // load's round trip runs beside a whole step's arithmetic; pv = 1: nothing waits
        auto *pm = seen;
        uint8_t pv = 1;
        for (int it = 0; it < N; ++it) {
            auto *m = seen;
            uint8_t v = 1;
            if ((unsigned)c0 < (unsigned)px && (unsigned)c1 < (unsigned)px && (unsigned)c2 < (unsigned)nz) {
                m = seen + ((size_t)c2 * px + (size_t)(px - 1 - c1)) * px + c0;
                if (ALWAYS_STORE) *m = 1; else v = *m;
            } else if ((c0 < 0 && st0 <= 0) || (c0 >= px && st0 >= 0) || (c1 < 0 && st1 <= 0) || (c1 >= px && st1 >= 0) ||
                       (c2 < 0 && st2 <= 0) || (c2 >= nz && st2 >= 0)) {
                break;                                      // integer early exit 2: outside on an axis and moving away, or not moving
            }
            if (pv == 0) *pm = 1;
            pm = m; pv = v;
            if (t0 <= t1 && t0 <= t2) {
                c0 += st0; --n0;
                t0 = n0 ? t0 + dl0 : INF;
            } else if (t1 <= t2) {
                c1 += st1; --n1;
                t1 = n1 ? t1 + dl1 : INF;
            } else {
                c2 += st2; --n2;
                t2 = n2 ? t2 + dl2 : INF;
            }
        }
        if (pv == 0) *pm = 1;
    }

    // the counters: wave, LDS, one global add per counter
    const uint32_t w_considered = wave_reduce_add(n_considered), w_cast = wave_reduce_add(n_cast);
    const uint32_t w_not_finite = wave_reduce_add(n_not_finite), w_too_long = wave_reduce_add(n_too_long);
    if ((tid & 63) == 0) {
        atomicAdd(&s_stat[0], (unsigned long long)w_considered);
        atomicAdd(&s_stat[1], (unsigned long long)w_cast);
        atomicAdd(&s_stat[2], (unsigned long long)w_not_finite);
        atomicAdd(&s_stat[3], (unsigned long long)w_too_long);
    }
    __syncthreads();
    if (tid < 4 && a.stats && s_stat[tid]) atomicAdd(a.stats + tid, s_stat[tid]);
}

static const WindowPass RAY_PASS = {"bev voxel rays", false, false};

extern "C" {

int pca_bev_voxel_rays(pca_ctx *ctx, const pca_store *store, const int64_t *frame_off, int slot_begin, int slot_end,
                       int64_t max_points, const pca_bev_params *prm, double z_lo, double z_step, int nz, int include_dyn,
                       const double *origins, const double *pending_Ts, const int *pending_slot_ends, int n_pending,
                       uint8_t *seen, int64_t *stats, void *stream)
{
    if (!ctx) return -1;
    if (max_points < 1) max_points = 1;
    hipStream_t s = (hipStream_t)stream;
    // every check comes before the first launch (a noted K1 and the clearing of the outputs included)
    RayArgs A;
    if (window_check(ctx, RAY_PASS, origins && (seen || stats), store, frame_off, slot_begin, slot_begin, slot_end, max_points, prm,
                     pending_Ts, pending_slot_ends, n_pending, A))
        return -1;
    if (voxel_grid_check(ctx, RAY_PASS.what, z_lo, z_step, nz)) return -1;
    A.z_lo = z_lo; A.z_step = z_step;
    A.nz = nz; A.include_dyn = include_dyn;
    A.G = point_pass_G(max_points, "PCA_BEV_RAYS_G");
    A.origins = origins;
    A.seen = seen;
    A.stats = reinterpret_cast<unsigned long long *>(stats);
    PCA_CHECK(ctx, hipSetDevice(ctx->device));
    if (pca_k1_flush_pending(ctx)) return -1;               // a noted K1 runs on its own first, as before the occupancy labels
    if (seen) PCA_CHECK(ctx, hipMemsetAsync(seen, 0, (size_t)nz * prm->px * prm->px, s));
    if (stats) PCA_CHECK(ctx, hipMemsetAsync(stats, 0, 4 * sizeof(int64_t), s));
    const RayArgs &args = A;
    if (slot_end > slot_begin)                              // (a window without a slot: no launch over zero points)
    {
        if (pca_env_int("PCA_BEV_RAYS_STORE", 0, 0, 1))     // A/B: 1 = every mark stores, without the load in front (same result)
            PCA_LAUNCH(ctx, PCA_K_BEV_VOXEL_RAYS, bev_voxel_rays<true>, dim3(args.G), dim3(POINT_THREADS), s, args);
        else
            PCA_LAUNCH(ctx, PCA_K_BEV_VOXEL_RAYS, bev_voxel_rays<false>, dim3(args.G), dim3(POINT_THREADS), s, args);
    }
    PCA_CHECK(ctx, hipGetLastError());
    return 0;
}

}  // extern "C"
