// pca_bev_ray_setup.h -- what the two passes that cast lidar rays through the voxel grid share (the marks of pca_bev_rays.hip, the
// crossing counts of pca_bev_carve.hip): the grid coordinates of a position and the set-up of one ray -- its start and end voxel,
// the integer step counts that drive the traversal, tMax and tDelta.  The ONE copy of each: the numpy model of
// tests/voxel_rays_common.py restates these expressions bit for bit, and both passes are held to it.
// Everything is f64, each operation rounded on its own (-ffp-contract=off), the product sum UNFUSED, the divisions IEEE.
#pragma once
#include "pca_bev_view.h"

#define RAY_COORD_LIM 1073741824.0   // 2^30: a grid coordinate at or above it in magnitude drops the ray

struct RayGrid { double ox, oy, oz, r0, r1, r3, r4, dx, dy, view, pxd, half_px, z_lo, z_step; };
__device__ __forceinline__ RayGrid ray_grid(const pca_bev_params &prm, double z_lo, double z_step)
{
    RayGrid q;
    q.ox = prm.origin[0]; q.oy = prm.origin[1]; q.oz = prm.origin[2];
    q.r0 = prm.R[0]; q.r1 = prm.R[1]; q.r3 = prm.R[3]; q.r4 = prm.R[4];
    q.dx = prm.dx; q.dy = prm.dy; q.view = prm.view;
    q.pxd = (double)prm.px; q.half_px = 0.5 * q.pxd;
    q.z_lo = z_lo; q.z_step = z_step;
    return q;
}
// grid coordinates of a position: each operation rounded on its own (-ffp-contract=off), the sums unfused
__device__ __forceinline__ void ray_coords(const RayGrid &q, double X, double Y, double Z, double &u, double &v, double &w)
{
    const double x = X - q.ox, y = Y - q.oy;
    const double ax = (q.r0 * x + q.r1 * y) + q.dx;
    const double ay = (q.r3 * x + q.r4 * y) + q.dy;
    u = ax / q.view * q.pxd + q.half_px;
    v = ay / q.view * q.pxd + q.half_px;
    w = (((Z - q.oz) + 0.0) - q.z_lo) / q.z_step;
}
__device__ __forceinline__ bool ray_coord_ok(double t) { return fabs(t) < RAY_COORD_LIM; }   // (false for NaN)

// One ray from grid coordinates s to e (all six ray_coord_ok).  c: the current voxel, the start voxel at first; g: the end voxel;
// n: the steps left per axis (each below 2^31: |c|, |g| <= 2^30).
struct RayVoxels { int c0, c1, c2, g0, g1, g2, n0, n1, n2; };
__device__ __forceinline__ RayVoxels ray_voxels(double s0, double s1, double s2, double e0, double e1, double e2)
{
    RayVoxels r;
    r.c0 = (int)floor(s0); r.c1 = (int)floor(s1); r.c2 = (int)floor(s2);
    r.g0 = (int)floor(e0); r.g1 = (int)floor(e1); r.g2 = (int)floor(e2);
    r.n0 = abs(r.g0 - r.c0); r.n1 = abs(r.g1 - r.c1); r.n2 = abs(r.g2 - r.c2);
    return r;
}
__device__ __forceinline__ int64_t ray_steps(const RayVoxels &r) { return (int64_t)r.n0 + r.n1 + r.n2; }
// the ray's voxel bounding box misses the grid: no step of it is inside
__device__ __forceinline__ bool ray_box_misses(const RayVoxels &r, int px, int nz)
{
    return (r.c0 < 0 && r.g0 < 0) || (r.c0 >= px && r.g0 >= px) || (r.c1 < 0 && r.g1 < 0) || (r.c1 >= px && r.g1 >= px) ||
           (r.c2 < 0 && r.g2 < 0) || (r.c2 >= nz && r.g2 >= nz);
}
// Amanatides-Woo, driven by the integer step counts: st the step per axis, t = tMax, dl = tDelta
struct RayMarch { int st0, st1, st2; double t0, t1, t2, dl0, dl1, dl2; };
__device__ __forceinline__ RayMarch ray_march(const RayVoxels &r, double s0, double s1, double s2, double e0, double e1, double e2)
{
    const double INF = __builtin_huge_val();
    RayMarch m;
    m.st0 = (r.g0 > r.c0) - (r.g0 < r.c0); m.st1 = (r.g1 > r.c1) - (r.g1 < r.c1); m.st2 = (r.g2 > r.c2) - (r.g2 < r.c2);
    const double d0 = e0 - s0, d1 = e1 - s1, d2 = e2 - s2;
    m.t0 = INF; m.t1 = INF; m.t2 = INF; m.dl0 = 0.0; m.dl1 = 0.0; m.dl2 = 0.0;
    if (r.n0 > 0) { m.t0 = ((double)(r.c0 + (m.st0 > 0 ? 1 : 0)) - s0) / d0; m.dl0 = 1.0 / fabs(d0); }
    if (r.n1 > 0) { m.t1 = ((double)(r.c1 + (m.st1 > 0 ? 1 : 0)) - s1) / d1; m.dl1 = 1.0 / fabs(d1); }
    if (r.n2 > 0) { m.t2 = ((double)(r.c2 + (m.st2 > 0 ? 1 : 0)) - s2) / d2; m.dl2 = 1.0 / fabs(d2); }
    return m;
}
// one step: the axis with the smallest tMax, ties in the order (u, v, w); an axis whose steps are used up never wins again
__device__ __forceinline__ void ray_advance(RayVoxels &r, RayMarch &m)
{
    const double INF = __builtin_huge_val();
    if (m.t0 <= m.t1 && m.t0 <= m.t2) {
        r.c0 += m.st0; --r.n0;
        m.t0 = r.n0 ? m.t0 + m.dl0 : INF;
    } else if (m.t1 <= m.t2) {
        r.c1 += m.st1; --r.n1;
        m.t1 = r.n1 ? m.t1 + m.dl1 : INF;
    } else {
        r.c2 += m.st2; --r.n2;
        m.t2 = r.n2 ? m.t2 + m.dl2 : INF;
    }
}
// outside the grid on an axis and moving away from it, or not moving on it: no later step of the ray is inside
__device__ __forceinline__ bool ray_gone(const RayVoxels &r, const RayMarch &m, int px, int nz)
{
    return (r.c0 < 0 && m.st0 <= 0) || (r.c0 >= px && m.st0 >= 0) || (r.c1 < 0 && m.st1 <= 0) || (r.c1 >= px && m.st1 >= 0) ||
           (r.c2 < 0 && m.st2 <= 0) || (r.c2 >= nz && m.st2 >= 0);
}
