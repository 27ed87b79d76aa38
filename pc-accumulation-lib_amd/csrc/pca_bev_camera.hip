// pca_bev_camera.hip -- camera rays cast through the voxel grid of the occupancy labels (pca_bev_voxel.hip): which voxels a
// pinhole camera sees before its ray is stopped by an occupied one -- the "mask_camera" of Occ3D, the ".occluded" of
// SemanticKITTI-SSC / SSCBench-KITTI-360 -- and, per ray, the first occupied voxel, its depth and its label.
//
//   bev_camera_rays  one thread per pixel ray, 256 threads, a grid-stride loop over the nu x nv rays (ray r: column r % nu, row
//                    r / nu; a wave holds 64 neighbouring pixels of a row, whose rays share cache lines of the label volume).
//                    The ray runs from the camera centre C to the point at camera depth max_depth; its grid coordinates and
//                    its set-up (voxels, step counts, tMax, tDelta) come from pca_bev_ray_setup.h, shared with
//                    pca_bev_rays.hip and pca_bev_carve.hip, and the walk is theirs (ray_advance, ties u, v, w) -- but it
//                    visits the end voxel too, reads the label of every voxel it visits inside the grid and stops at the
//                    first one that is not 255.  A mark is a byte load and, where that reads 0, a byte store of 1: every
//                    writer writes the same value, so no atomic is needed and the result does not depend on the order.
//                    The label decides whether the ray goes on, so a walk that tests each voxel before it steps waits one L2
//                    round trip per step (DEPTH = 1, the plain form).  DEPTH > 1 breaks that chain: the walk is driven by
//                    integers and needs no label, so the next DEPTH voxels are computed first, their label and mark bytes
//                    loaded together -- every load unconditional, an absent voxel reads byte 0 of the volume and its value is
//                    discarded -- and only then tested in order; the marks behind a hit are suppressed, so the result is
//                    that of the plain form bit for bit (profiles/bev_voxel_camera.txt has both).  The camera's own voxel is
//                    tested alone first, so that a camera inside an occupied voxel costs what it costs in the plain form.
//                    The five counters: per lane, then point_count (pca_point_pass.h).
// The entry reads no store and no owed chain, and writes only its outputs.  PCA_BEV_RAYS_MAX_STEPS bounds every ray, hence every
// launch.
#include "pca_bev_ray_setup.h"
#include "pca_point_pass.h"

#define CAMERA_DEPTH_DEFAULT 4    // voxels whose bytes are loaded before the first of them is tested

struct alignas(16) CameraArgs {
    pca_bev_params prm;
    double z_lo, z_step;
    double Minv[9], C[3], max_depth;
    int nz, nu, nv, stride;
    int G;                        // workgroups of the launch
    const uint8_t *labels;        // [nz][px][px], 255 = empty
    uint8_t *visible;             // [nz][px][px]
    int32_t *hit;                 // [nv][nu] or NULL
    float *depth;                 // [nv][nu] or NULL
    uint8_t *label;               // [nv][nu] or NULL
    unsigned long long *stats;    // [5]
};

// One ray's walk: r, m the traversal's state at the current voxel; left: the steps behind it; t_enter: the parameter at which
// it was entered; the hit so far (-1: none).
struct CameraWalk { RayVoxels r; RayMarch m; int left; double t_enter; bool walking; int32_t hit; double t_hit; uint8_t hit_label; };
typedef __attribute__((address_space(1))) uint8_t CameraBytes;

// The next D voxels of the walk: computed first, their bytes loaded together, then tested in order.
template <int D>
__device__ __forceinline__ void camera_batch(CameraWalk &w, const CameraBytes *labels, CameraBytes *visible, int px, int nz)
{
    // place (-1: outside the grid, or the walk has ended) and entry parameter
    int place[D];
    double t_in[D];
#pragma unroll
    for (int b = 0; b < D; ++b) {
        place[b] = -1;
        t_in[b] = w.t_enter;
        if (w.walking) {
            const RayVoxels &r = w.r;
            const bool inside = (unsigned)r.c0 < (unsigned)px && (unsigned)r.c1 < (unsigned)px && (unsigned)r.c2 < (unsigned)nz;
            if (inside) place[b] = (r.c2 * px + (px - 1 - r.c1)) * px + r.c0;
            if (w.left == 0 || (!inside && ray_gone(r, w.m, px, nz))) {     // (ray_gone: integer early exit 2)
                w.walking = false;
            } else {
                const RayMarch &m = w.m;
                w.t_enter = (m.t0 <= m.t1 && m.t0 <= m.t2) ? m.t0 : (m.t1 <= m.t2 ? m.t1 : m.t2);   // the axis ray_advance steps
                ray_advance(w.r, w.m);
                --w.left;
            }
        }
    }
    // their bytes, all loads issued before the first test (unconditional: an absent voxel reads byte 0, its value is dropped)
    uint8_t lab[D], vis[D];
#pragma unroll
    for (int b = 0; b < D; ++b) {
        const int at = place[b] < 0 ? 0 : place[b];
        lab[b] = labels[at];
        vis[b] = visible[at];
    }
#pragma unroll
    for (int b = 0; b < D; ++b) {
        if (place[b] >= 0 && w.hit < 0) {                   // (behind a hit nothing is marked)
            if (vis[b] == 0) visible[place[b]] = 1;
            if (lab[b] != 255) {
                w.hit = place[b];
                w.t_hit = t_in[b];
                w.hit_label = lab[b];
            }
        }
    }
    if (w.hit >= 0) w.walking = false;
}

template <int DEPTH>
__global__ __launch_bounds__(POINT_THREADS) void bev_camera_rays(const CameraArgs a)
{
    const RayGrid q = ray_grid(a.prm, a.z_lo, a.z_step);
    const int px = a.prm.px, nz = a.nz, nu = a.nu;
    const int64_t rays = (int64_t)a.nu * a.nv;
    const double half = (double)(a.stride - 1) / 2.0, depth_max = a.max_depth;
    auto *visible = reinterpret_cast<CameraBytes *>(reinterpret_cast<uintptr_t>(a.visible));
    auto *labels = reinterpret_cast<const CameraBytes *>(reinterpret_cast<uintptr_t>(a.labels));
    // the camera centre is every ray's start
    double s0, s1, s2;
    ray_coords(q, a.C[0], a.C[1], a.C[2], s0, s1, s2);
    const bool s_ok = ray_coord_ok(s0) && ray_coord_ok(s1) && ray_coord_ok(s2);
    uint32_t n_rays = 0, n_cast = 0, n_not_finite = 0, n_too_long = 0, n_hits = 0;

    for (int64_t ray = (int64_t)blockIdx.x * POINT_THREADS + threadIdx.x; ray < rays; ray += (int64_t)a.G * POINT_THREADS) {
        ++n_rays;
        int32_t hit = -1;
        double t_hit = 0.0;
        uint8_t hit_label = 255;
        const int64_t pj = ray / nu;
        const double u = (double)((ray - pj * nu) * a.stride) + half, v = (double)(pj * a.stride) + half;
        const double d0 = (a.Minv[0] * u + a.Minv[1] * v) + a.Minv[2];
        const double d1 = (a.Minv[3] * u + a.Minv[4] * v) + a.Minv[5];
        const double d2 = (a.Minv[6] * u + a.Minv[7] * v) + a.Minv[8];
        double e0, e1, e2;
        ray_coords(q, a.C[0] + depth_max * d0, a.C[1] + depth_max * d1, a.C[2] + depth_max * d2, e0, e1, e2);
        if (!(s_ok && ray_coord_ok(e0) && ray_coord_ok(e1) && ray_coord_ok(e2))) {
            ++n_not_finite;
        } else {
            const RayVoxels r = ray_voxels(s0, s1, s2, e0, e1, e2);
            const int64_t N64 = ray_steps(r);
            if (N64 > PCA_BEV_RAYS_MAX_STEPS) {
                ++n_too_long;
            } else {
                ++n_cast;
                if (!ray_box_misses(r, px, nz)) {           // integer early exit 1
                    CameraWalk w = {r, ray_march(r, s0, s1, s2, e0, e1, e2), (int)N64, 0.0, true, -1, 0.0, 255};
                    // the camera's own voxel alone first: a ray that is stopped there costs what it costs in the plain form
                    if constexpr (DEPTH > 1) camera_batch<1>(w, labels, visible, px, nz);
                    while (w.walking) camera_batch<DEPTH>(w, labels, visible, px, nz);
                    hit = w.hit; t_hit = w.t_hit; hit_label = w.hit_label;
                }
            }
        }
        if (hit >= 0) ++n_hits;
        if (a.hit) a.hit[ray] = hit;
        if (a.depth) a.depth[ray] = hit >= 0 ? (float)(t_hit * depth_max) : 0.0f;
        if (a.label) a.label[ray] = hit_label;
    }
    point_count(a.stats, n_rays, n_cast, n_not_finite, n_too_long, n_hits);
}

extern "C" {

int pca_bev_voxel_camera(pca_ctx *ctx, const pca_bev_params *prm, double z_lo, double z_step, int nz, const uint8_t *labels,
                         const pca_ray_camera *cam, uint8_t *visible, int32_t *hit, float *depth, uint8_t *label, int64_t *stats,
                         void *stream)
{
    if (!ctx) return -1;
    hipStream_t s = (hipStream_t)stream;
    const std::string w("bev voxel camera");
    // every check comes before the first launch (the clearing of the outputs included)
    if (!prm) { ctx->err = w + ": prm must not be NULL"; return -1; }
    if (!labels) { ctx->err = w + ": labels must not be NULL"; return -1; }
    if (!cam) { ctx->err = w + ": cam must not be NULL"; return -1; }
    if (!visible) { ctx->err = w + ": visible must not be NULL"; return -1; }
    if (!stats) { ctx->err = w + ": stats must not be NULL"; return -1; }
    if (cam->width < 1 || cam->height < 1) { ctx->err = w + ": width and height must be >= 1"; return -1; }
    if (cam->stride < 1 || cam->stride > (cam->width < cam->height ? cam->width : cam->height)) {
        ctx->err = w + ": stride must be in 1..min(width, height)";
        return -1;
    }
    if (!(cam->max_depth > 0.0 && cam->max_depth < __builtin_huge_val())) {     // (false for a NaN)
        ctx->err = w + ": max_depth must be finite and > 0";
        return -1;
    }
    for (int i = 0; i < 9; ++i)
        if (!(fabs(cam->Minv[i]) < __builtin_huge_val())) { ctx->err = w + ": every entry of Minv must be finite"; return -1; }
    for (int i = 0; i < 3; ++i)
        if (!(fabs(cam->C[i]) < __builtin_huge_val())) { ctx->err = w + ": every entry of C must be finite"; return -1; }
    if (voxel_grid_check(ctx, w.c_str(), z_lo, z_step, nz)) return -1;
    if (prm->px < 1 || prm->px > SIDE_PX_MAX) { ctx->err = w + ": px must be in 1..1024"; return -1; }
    if (bev_check_rotation(ctx, w.c_str(), prm)) return -1;
    CameraArgs A;
    A.prm = *prm;
    A.z_lo = z_lo; A.z_step = z_step;
    for (int i = 0; i < 9; ++i) A.Minv[i] = cam->Minv[i];
    for (int i = 0; i < 3; ++i) A.C[i] = cam->C[i];
    A.max_depth = cam->max_depth;
    A.nz = nz; A.stride = cam->stride;
    A.nu = cam->width / cam->stride; A.nv = cam->height / cam->stride;      // (both >= 1: stride <= min(width, height))
    A.G = point_pass_G((int64_t)A.nu * A.nv, "PCA_BEV_CAMERA_G");
    A.labels = labels;
    A.visible = visible; A.hit = hit; A.depth = depth; A.label = label;
    A.stats = reinterpret_cast<unsigned long long *>(stats);
    PCA_CHECK(ctx, hipSetDevice(ctx->device));
    if (cam->clear) PCA_CHECK(ctx, hipMemsetAsync(visible, 0, (size_t)nz * prm->px * prm->px, s));
    PCA_CHECK(ctx, hipMemsetAsync(stats, 0, 5 * sizeof(int64_t), s));
    const CameraArgs &args = A;
    // A/B: voxels loaded before the first is tested; 1 = the plain form, every step waits for its own label (same result)
    switch ((int)pca_env_int("PCA_BEV_CAMERA_DEPTH", CAMERA_DEPTH_DEFAULT, 1, 8)) {
    case 1: PCA_LAUNCH(ctx, PCA_K_BEV_CAMERA_RAYS, bev_camera_rays<1>, dim3(args.G), dim3(POINT_THREADS), s, args); break;
    case 2: PCA_LAUNCH(ctx, PCA_K_BEV_CAMERA_RAYS, bev_camera_rays<2>, dim3(args.G), dim3(POINT_THREADS), s, args); break;
    case 8: PCA_LAUNCH(ctx, PCA_K_BEV_CAMERA_RAYS, bev_camera_rays<8>, dim3(args.G), dim3(POINT_THREADS), s, args); break;
    default: PCA_LAUNCH(ctx, PCA_K_BEV_CAMERA_RAYS, bev_camera_rays<4>, dim3(args.G), dim3(POINT_THREADS), s, args); break;
    }
    PCA_CHECK(ctx, hipGetLastError());
    return 0;
}

}  // extern "C"
