// pca_render.hip -- the window of the store rendered into a pinhole camera: a z-buffer over the stored points (dense depth,
// colour and class targets for an image, as accumulated lidar projected with velo2img gives them).  The first pass of the
// read-only family (pca_bev_view.h) whose output is not a BEV grid.
//
//   render_zbuffer   one thread per stored point of the window, 256 threads, a grid-stride loop over chunks of 256 points.
//                    The point (owed re-transforms applied: pca_bev_view.h) is projected with K1's expressions
//                    (render_project below) and, where the mask keeps it, the key  float_bits((float)d) << 32 | window index  goes by
//                    an unsigned 64-bit atomic minimum into every pixel of its (2 radius + 1)^2 footprint, clipped to the
//                    image.  The bits of a non-negative float are monotone in its value: the minimum is the smallest depth
//                    rounded to f32 and, among equal depths, the smallest window index -- whatever the order of arrival.
//                    A pixel's key is read with a plain load first and the atomic issued only where the key is below it: keys
//                    only ever fall, so a stale value costs a redundant atomic and never loses a minimum (ALWAYS_ATOMIC:
//                    the A/B form without the load, same result).  The two counters: per lane, then point_count.
//   render_resolve   one thread per pixel: the key taken apart into depth and index, colour and class gathered from the
//                    winner's rgbs word; the covered pixels counted the same way.
// The window, its cuts and the counters' way to memory are those of pca_point_pass.h.  The store is never written.
#include "pca_point_pass.h"

#define RENDER_MAX_PIXELS (1 << 24)
#define RENDER_MAX_RADIUS 3
#define RENDER_EMPTY 0xffffffffffffffffull

struct alignas(16) RenderArgs {
    pca_store st;
    const int64_t *frame_off;
    int slot_begin, slot_end;
    int64_t max_points;
    BevOwed owed;                 // owed re-transforms: applied to the points that are read, never written back
    Mat34 P;                      // store coordinates -> image
    int W, H, radius, include_dyn;
    double min_depth, max_depth;
    ClassMask only;               // the classes that take part (use_only)
    int use_only;
    int G;                        // workgroups of render_zbuffer
    unsigned long long *keys;     // [H][W]
    float *depth;
    int64_t *index;
    uint8_t *rgb, *sem;
    unsigned long long *stats;    // [3]
    uint32_t *status;             // context status word (PCA_STATUS_* bits)
};

// velo2frame + velo2img of one point (sem_pc_accum.py:347-394): the eight lines of k1_project_pixel (pca_k1_body.h) RESTATED
// on f64 inputs, with the depth range in place of 0 and +inf.  Not one shared copy: with the body factored out of K1, K1's
// device assembly changed, and K1 is tuned as it stands.  tests/test_render_camera_model.py ties these expressions, through
// the numpy model, to the oracle K1 is held to.
struct RenderProj { double uf, vf, d; };
__device__ __forceinline__ RenderProj render_project(const Mat34 &P, double x, double y, double z)
{
    const double fx = row4(P.m + 0, x, y, z);
    const double fy = row4(P.m + 4, x, y, z);
    double d = row4(P.m + 8, x, y, z);
    if (d == 0.0) d = -1e-6;
    const double ad = fabs(d);
    const double qu = fx / ad, qv = fy / ad;
    return {rint(qu), rint(qv), d};
}
// the reference's mask with the depth range (0 and +inf: the reference's own); false for any NaN
__device__ __forceinline__ bool render_inside(const RenderProj &q, int W, int H, double d_lo, double d_hi)
{
    return (q.uf >= 0.0) && (q.uf < (double)W) && (q.vf >= 0.0) && (q.vf < (double)H) && (q.d > d_lo) && (q.d < d_hi);
}

template <bool ALWAYS_ATOMIC>
__global__ __launch_bounds__(POINT_THREADS) void render_zbuffer(const RenderArgs a)
{
    const int tid = (int)threadIdx.x;
    const PointWindow w = point_window<true>(a);
    const int64_t lo = w.lo, hi = w.hi;
    const PendHi pend_hi = owed_bounds(a.owed, a.frame_off, a.slot_begin, lo);
    const int W = a.W, H = a.H, rad = a.radius;
    auto *keys = reinterpret_cast<__attribute__((address_space(1))) unsigned long long *>(reinterpret_cast<uintptr_t>(a.keys));
    uint32_t n_considered = 0, n_kept = 0;

    for (int64_t p = lo + (int64_t)blockIdx.x * POINT_THREADS + tid; p < hi; p += (int64_t)a.G * POINT_THREADS) {
        if (!a.include_dyn && pca_ldg(a.st.dyn + p) == 1) continue;
        if (a.use_only && !in_mask(a.only, pca_ldg(a.st.rgbs + p) >> 24)) continue;
        ++n_considered;
        double X = pca_ldg(a.st.x + p), Y = pca_ldg(a.st.y + p), Z = pca_ldg(a.st.z + p);
        apply_owed(a.owed, pend_hi, p, X, Y, Z);
        const RenderProj q = render_project(a.P, X, Y, Z);
        if (!render_inside(q, W, H, a.min_depth, a.max_depth)) continue;
        ++n_kept;
        const int u = (int)q.uf, v = (int)q.vf;
        const unsigned long long key = ((unsigned long long)__float_as_uint((float)q.d) << 32) | (uint32_t)(p - lo);
        // the footprint, clipped to the image (the centre is inside: no range is empty)
        const int u0 = u - rad < 0 ? 0 : u - rad, u1 = u + rad > W - 1 ? W - 1 : u + rad;
        const int v0 = v - rad < 0 ? 0 : v - rad, v1 = v + rad > H - 1 ? H - 1 : v + rad;
        for (int vv = v0; vv <= v1; ++vv)
            for (int uu = u0; uu <= u1; ++uu) {
                auto *k = keys + ((size_t)vv * W + uu);
                if (ALWAYS_ATOMIC || key < *k)
                    __hip_atomic_fetch_min(k, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
    }
    point_count(a.stats, n_considered, n_kept);
}

__global__ __launch_bounds__(POINT_THREADS) void render_resolve(const RenderArgs a)
{
    const int64_t lo = point_window<false>(a).lo;
    const int64_t pix = (int64_t)blockIdx.x * POINT_THREADS + threadIdx.x;
    uint32_t covered = 0;
    if (pix < (int64_t)a.W * a.H) {
        const unsigned long long key = pca_ldg(a.keys + pix);
        float depth = 0.0f;
        int64_t index = -1;
        uint32_t c = 255u << 24;                            // rgb 0, 0, 0 and class 255: nothing was seen
        if (key != RENDER_EMPTY) {
            depth = __uint_as_float((uint32_t)(key >> 32));
            index = (int64_t)(uint32_t)key;
            c = pca_ldg(a.st.rgbs + lo + index);            // (an index a kept point wrote: below the window's cut end)
            covered = 1;
        }
        a.depth[pix] = depth;
        a.index[pix] = index;
        a.rgb[pix * 3 + 0] = (uint8_t)c;
        a.rgb[pix * 3 + 1] = (uint8_t)(c >> 8);
        a.rgb[pix * 3 + 2] = (uint8_t)(c >> 16);
        a.sem[pix] = (uint8_t)(c >> 24);
    }
    point_count(a.stats + 2, covered);
}

static const WindowPass RENDER_PASS = {"render camera", true, false};

extern "C" {

int pca_render_camera(pca_ctx *ctx, const pca_store *store, const int64_t *frame_off, int slot_begin, int slot_end,
                      int64_t max_points, const pca_camera *cam, const pca_class_group *only, const double *pending_Ts,
                      const int *pending_slot_ends, int n_pending, uint64_t *keys, float *depth, int64_t *index, uint8_t *rgb,
                      uint8_t *sem, int64_t *stats, void *stream)
{
    if (!ctx) return -1;
    if (max_points < 1) max_points = 1;
    hipStream_t s = (hipStream_t)stream;
    // every check comes before the first launch (a noted K1 and the clearing of the outputs included)
    RenderArgs A;
    if (window_check_any(ctx, RENDER_PASS, cam && keys && depth && index && rgb && sem && stats, store, frame_off, slot_begin,
                         slot_begin, slot_end, max_points, []() { return 0; }, pending_Ts, pending_slot_ends, n_pending, A))
        return -1;
    const std::string w(RENDER_PASS.what);
    if (cam->width < 1 || cam->height < 1 || (int64_t)cam->width * cam->height > RENDER_MAX_PIXELS) {
        ctx->err = w + ": need 1 <= width, height and width * height <= 16777216";
        return -1;
    }
    if (cam->radius < 0 || cam->radius > RENDER_MAX_RADIUS) { ctx->err = w + ": radius must be in 0..3"; return -1; }
    if (!(cam->min_depth >= 0.0 && cam->min_depth < cam->max_depth)) {      // (false for a NaN)
        ctx->err = w + ": need 0 <= min_depth < max_depth";
        return -1;
    }
    for (int i = 0; i < 12; ++i)
        if (!(fabs(cam->P[i]) < __builtin_huge_val())) { ctx->err = w + ": every entry of P must be finite"; return -1; }
    if (max_points >= (1ll << 32)) { ctx->err = w + ": max_points must be below 2^32 (the window index is 32 bits wide)"; return -1; }
    for (int i = 0; i < 12; ++i) A.P.m[i] = cam->P[i];
    A.W = cam->width; A.H = cam->height; A.radius = cam->radius; A.include_dyn = cam->include_dyn;
    A.min_depth = cam->min_depth; A.max_depth = cam->max_depth;
    for (int i = 0; i < 4; ++i) A.only.w[i] = only ? only->mask[i] : 0;
    A.use_only = only ? 1 : 0;
    A.G = point_pass_G(max_points, "PCA_RENDER_G");
    A.keys = reinterpret_cast<unsigned long long *>(keys);
    A.depth = depth; A.index = index; A.rgb = rgb; A.sem = sem;
    A.stats = reinterpret_cast<unsigned long long *>(stats);
    const size_t pixels = (size_t)A.W * A.H;
    PCA_CHECK(ctx, hipSetDevice(ctx->device));
    if (pca_k1_flush_pending(ctx)) return -1;               // a noted K1 runs on its own first, as before the rays
    PCA_CHECK(ctx, hipMemsetAsync(keys, 0xFF, pixels * sizeof(uint64_t), s));
    PCA_CHECK(ctx, hipMemsetAsync(stats, 0, 3 * sizeof(int64_t), s));
    const RenderArgs &args = A;
    if (slot_end > slot_begin)                              // (a window without a slot: no launch over zero points)
    {
        if (pca_env_int("PCA_RENDER_ALWAYS_ATOMIC", 0, 0, 1))   // A/B: 1 = every pixel of a footprint gets its atomic (same result)
            PCA_LAUNCH(ctx, PCA_K_RENDER_ZBUFFER, render_zbuffer<true>, dim3(args.G), dim3(POINT_THREADS), s, args);
        else
            PCA_LAUNCH(ctx, PCA_K_RENDER_ZBUFFER, render_zbuffer<false>, dim3(args.G), dim3(POINT_THREADS), s, args);
    }
    PCA_LAUNCH(ctx, PCA_K_RENDER_RESOLVE, render_resolve, dim3((unsigned)((pixels + POINT_THREADS - 1) / POINT_THREADS)),
               dim3(POINT_THREADS), s, args);
    PCA_CHECK(ctx, hipGetLastError());
    return 0;
}

}  // extern "C"
