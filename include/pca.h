/*
 * pca.h -- C ABI of the MI355X (gfx950) semantic point-cloud accumulator + BEV rasteriser.
 *
 * The reference (robin-karlsson0/pc-accumulation-lib) is pure Python and has no FFI layer: its
 * "plugin interface" for this path is the Python classes in sem_pc_accum.py / bev_generator/.  This
 * header is the boundary a maintainer binds underneath those classes (ctypes stub: INTEGRATION.md);
 * every entry point names the reference code it replaces (file:line relative to the reference root).
 *
 * Conventions
 *   - all pointers marked "dev" are device (HBM) pointers, everything else is host memory read
 *     synchronously during the call;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls only enqueue work and
 *     never synchronise unless stated;
 *   - return value 0 = ok, negative = error (text via pca_last_error); no exceptions cross the boundary;
 *   - one pca_ctx per host thread / GPU; calls on one ctx must target one stream at a time.
 *
 * Point store (HBM layout): structure-of-arrays, 37 B per stored point
 *     x,y,z      f64   reference sem_pc columns 0..2
 *     intensity  f32   RAW lidar intensity; column 3 = raw (KITTI) or raw/255. (NuScenes), the division
 *                      is applied by consumers (pca_bev_params.intensity_div255) exactly as the reference's
 *                      f64 division would
 *     rgbs       u32   r | g<<8 | b<<16 | sem<<24 (columns 4..7, small non-negative integers)
 *     inst       i32   column 8
 *     dyn        u8    column 9
 * Frames are contiguous segments; `frame_off` (dev, int64[max_frames+1]) holds the segment boundaries
 * and lives on the device so that integrate() never has to read a count back.
 */
#ifndef PCA_H
#define PCA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCA_VERSION 2

typedef struct pca_ctx pca_ctx;

typedef struct {
    double *x, *y, *z;   /* dev */
    float *intensity;    /* dev */
    uint32_t *rgbs;      /* dev */
    int32_t *inst;       /* dev */
    uint8_t *dyn;        /* dev */
    int64_t capacity;    /* points */
    /* Optional (version 2; NULL = absent): dev, six words per slot, ZEROED by the caller whenever a slot is (re)used.  K1 (one-frame
     * launches) leaves there the box of the points the frame kept, in the frame's own coordinates: words 2k / 2k+1 = lower /
     * upper bound of coordinate k as an order-preserving code of the f32 (pca_f32_box_decode turns a row into six floats;
     * upper word 0 = the frame kept nothing, or K1 has not run yet).  A caller that reads rows back -- whenever it likes: a row
     * it has not seen only means "unknown" -- can tell which frames cannot reach a raster's view (pca_host_view_hull,
     * pca_bev_bin_range). */
    uint32_t *frame_box;
} pca_store;

/* status bits accumulated on the device, read back with pca_status() */
#define PCA_STATUS_STORE_OVERFLOW 1u /* a kernel wanted to write past store.capacity (points dropped)     */
#define PCA_STATUS_UV_OUT_OF_IMAGE 2u /* NuScenes: pixel coords outside (1, wh-1): reference AssertionError */
#define PCA_STATUS_NEGATIVE_INTENSITY 4u /* BEV: a negative f32 intensity (pass intensity64 for such data)   */
#define PCA_STATUS_LOOKBACK_TIMEOUT 8u /* a compaction workgroup gave up waiting for a predecessor (output invalid) */
#define PCA_STATUS_LANES_BISECT_CAP 16u /* lanes: a border crossing was not found within 1100 halvings (row invalid) */

int pca_version(void);
int pca_ctx_create(int device, pca_ctx **out);
void pca_ctx_destroy(pca_ctx *ctx);
const char *pca_last_error(pca_ctx *ctx);
/* Synchronises `stream`, returns the OR of PCA_STATUS_* bits raised since the last call and clears them. */
int pca_status(pca_ctx *ctx, void *stream, uint32_t *status_out);
/* The same bits as the host can see them now, WITHOUT touching the stream (every raise also stores into a mapped host
 * word): a kernel's raise shows here at the latest once that kernel has finished.  Does not clear; pca_status does.
 * The drop-in classes peek on every integrate() / generate_bev() and where they wait for a result anyway, so that a
 * dropped point or an invalid compaction surfaces as the exception the reference would have raised synchronously
 * (IndexError of bev_generator/sem_bev.py:543-551, AssertionError of datasets/nuscenes_utils.py:191-195). */
int pca_status_peek(pca_ctx *ctx, uint32_t *status_out);
/* the mirror itself: host address of 8 words, word b != 0 <=> bit b raised (for bindings that want a zero-cost read) */
const uint32_t *pca_status_mirror(pca_ctx *ctx);

/* ------------------------------------------------------------------------------------------------
 * K1  KITTI-360 fused  project -> frustum mask -> nearest sample (rgb + semseg) -> class filter ->
 *     stable compaction -> append.   Replaces, per frame,
 *       sem_pc_accum.py:347-402 (velo2frame, velo2img), :323-345 (gen_semantic_pc, called twice from
 *       kitti360_sem_pc_accum.py:132-135), :317-321 (filter_semseg_pc), kitti360_sem_pc_accum.py:136-156.
 *     One launch handles a BATCH of frames (frame k appends into slot first_slot+k); kept points keep
 *     their input order (the reference's boolean-mask compaction is stable).
 *     If frame.sem_gt != NULL the use_gt_sem branch (kitti360_sem_pc_accum.py:139-144) is taken:
 *     no projection, rgb = 0, class = sem_gt[p].
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    const float *pts;      /* dev [n,4] f32 x,y,z,intensity                                    */
    const uint8_t *rgb;    /* dev [H,W,3] u8, or NULL with sem_gt                              */
    const uint8_t *sem;    /* dev [H,W]   u8 class map, or NULL with sem_gt                    */
    const uint8_t *sem_gt; /* dev [n] u8 per-point class, or NULL                              */
    int32_t n;             /* points in this frame                                             */
    int32_t reserved;      /* ignored                                                          */
} pca_kitti_frame;

/* frames: HOST array of n_frames descriptors (copied into the launch).  P: 3x4 row-major f64
 * (P_velo_frame).  filter_mask: 256-bit class set.  frame_off[first_slot] must hold the append position;
 * frame_off[first_slot+k+1] is written for every frame k. */
int pca_kitti_project_sample_filter(pca_ctx *ctx, const pca_kitti_frame *frames, int n_frames, const double P[12],
                                    int H, int W, const uint64_t filter_mask[4], const pca_store *store,
                                    int64_t *frame_off /*dev*/, int first_slot, void *stream);

/* Sample modes of K1 / K1n.  NEAREST is what the reference's callers use (sem_pc_accum.py:338-341 rounds the pixel,
 * nuscenes_oracle_sem_pc_accum.py:466-469 passes 'nearest').  BILINEAR is opt-in (the reference has the branch,
 * datasets/nuscenes_utils.py:197-210, but no caller): r, g, b = round-half-even of the bilinear mix of the four
 * neighbours, weights exactly as that branch computes them (pinned through pca_sample_bilinear), neighbours clamped to
 * the image, an integer coordinate takes floor + 1 as its upper neighbour (weight 0) instead of the reference's 0 / 0;
 * the class is always the nearest pixel's. */
#define PCA_SAMPLE_NEAREST 0
#define PCA_SAMPLE_BILINEAR 1
int pca_kitti_project_sample_filter_ex(pca_ctx *ctx, const pca_kitti_frame *frames, int n_frames, const double P[12],
                                       int H, int W, const uint64_t filter_mask[4], const pca_store *store,
                                       int64_t *frame_off /*dev*/, int first_slot, int sample_mode, void *stream);

/* ------------------------------------------------------------------------------------------------
 * K1n NuScenes (oracle pose)  nearest sample from 6 camera images -> invalid / class filter ->
 *     stable compaction -> ego->world transform -> append.
 *     Replaces nuscenes_oracle_sem_pc_accum.py:457-501 and datasets/nuscenes_utils.py:181-214 ('nearest').
 *     pc: dev [n,7] f64 rows x,y,z,intensity,u,v,inst;  cam_idx: dev [n] int64 (-1: on no image);
 *     imgs: dev [ncam,H,W,3] u8; sems: dev [ncam,H,W] u8;  T: host, 4x4 row-major f64 (T_ego_world), not NULL.
 *     A point whose cam_idx lies outside [0, ncam) is dropped silently, whatever its u, v (the reference never looks at
 *     them).  A point assigned to a camera whose u, v do not satisfy 1 < u < W - 1, 1 < v < H - 1 (on a bound, outside, NaN,
 *     +-inf, -0.0) raises PCA_STATUS_UV_OUT_OF_IMAGE and is DROPPED: the call stores exactly the rows it would store without
 *     that point, in both forms and both sample modes (the reference raises and stores nothing; the drop-in classes turn the
 *     bit into that AssertionError).  On PCA_STATUS_STORE_OVERFLOW the rows below store.capacity are the right ones,
 *     nothing at or behind it is written, and frame_off still counts every row the frame keeps: frame_off[slot + 1] =
 *     frame_off[slot] + kept, which may lie behind capacity.
 * ------------------------------------------------------------------------------------------------ */
int pca_nusc_sample_filter_transform(pca_ctx *ctx, const double *pc, const int64_t *cam_idx, int32_t n,
                                     const uint8_t *imgs, const uint8_t *sems, int ncam, int H, int W,
                                     const double T[16], const uint64_t filter_mask[4], const pca_store *store,
                                     int64_t *frame_off /*dev*/, int slot, void *stream);
int pca_nusc_sample_filter_transform_ex(pca_ctx *ctx, const double *pc, const int64_t *cam_idx, int32_t n,
                                        const uint8_t *imgs, const uint8_t *sems, int ncam, int H, int W,
                                        const double T[16], const uint64_t filter_mask[4], const pca_store *store,
                                        int64_t *frame_off /*dev*/, int slot, int sample_mode, void *stream);

/* The same for a BATCH of frames (a whole scene: run_nuscenes_bev_gen.py:236-237 integrates every sample of a scene before
 * the first BEV): one front launch over the tiles of all frames + one append launch, the stored rows being exactly those of
 * n_frames single calls in order (slots first_slot .. first_slot + n_frames - 1; the K3 marks of the tracker are applied
 * afterwards, in tracker order).  Every frame has its own point rows, camera indices, image stack and T_ego_world; the
 * image stacks share ncam, H, W.  At most 16384 tiles of 512 points per call. */
typedef struct {
    const double *pc;          /* dev [n,7] f64 rows x,y,z,intensity,u,v,inst */
    const int64_t *cam_idx;    /* dev [n] */
    const uint8_t *imgs;       /* dev [ncam,H,W,3] */
    const uint8_t *sems;       /* dev [ncam,H,W] */
    int32_t n;
    int32_t reserved;
    const double *T;           /* host 4x4 row-major f64 (T_ego_world) */
} pca_nusc_frame;
int pca_nusc_sample_filter_transform_batch(pca_ctx *ctx, const pca_nusc_frame *frames, int n_frames, int ncam, int H, int W,
                                           const uint64_t filter_mask[4], const pca_store *store, int64_t *frame_off /*dev*/,
                                           int first_slot, int sample_mode, void *stream);

/* pts_feat_from_img(pts_uv, img, method='bilinear') of the reference for a 2-D feature map (its bilinear branch only
 * works for those): datasets/nuscenes_utils.py:181-210, the arithmetic to the letter.  map: dev [H,W] f64; uv: dev [n,2]
 * f64 (u along x); out: dev [n] f64.  Raises PCA_STATUS_UV_OUT_OF_IMAGE where the reference's assert fails: that point's out
 * is 0.0, every other point's is what it is without it.  An integer u or v gives NaN (the reference's 0 / 0).  n = 0 returns
 * 0 and writes nothing. */
int pca_sample_bilinear(pca_ctx *ctx, const double *map /*dev*/, int H, int W, const double *uv /*dev*/, int32_t n,
                        double *out /*dev*/, void *stream);

/* ------------------------------------------------------------------------------------------------
 * K0n NuScenes lidar -> ego -> global -> N cameras, pinhole projection, last camera wins.
 *     Replaces obs_dataloaders/nuscenes_obs_dataloader.py:162-202 and
 *     datasets/nuscenes_utils.py:46-60, :112-136 (view_points = nuscenes-devkit, restated).
 *     pc_lidar dev [n,3] f64.  T_cam_from_glob [ncam,16], K [ncam,9], wh [ncam,2] host arrays.
 *     Outputs dev: pc_in_ego [n,3], uv [n,2] f64, cam_idx [n] int64.
 *     ncam: 0 .. 8, anything else returns -1 and writes nothing; ncam = 0 writes pc_in_ego, uv = 0 and cam_idx = -1.
 *     n <= 0 returns 0 and writes nothing.  With n > 0, pc_lidar, the two transforms and the three outputs must not be NULL,
 *     nor T_cam_from_glob, K and wh with ncam > 0 (-1, nothing launched).  A point is taken by camera j where cz > 1e-3, 1 < u < w_j - 1 and
 *     1 < v < h_j - 1, all strict; a point no camera takes (NaN and inf coordinates among them) keeps uv = 0, cam_idx = -1.
 *     Every output is bit-equal to the reference's but for the sign of a NaN the arithmetic itself produced (0 x inf,
 *     inf - inf in pc_in_ego of a point with an infinite coordinate): gfx950 clears it, x86 sets it.  The same holds for the
 *     0 / 0 of pca_sample_bilinear at an integer coordinate.  Such values never reach the store.
 * ------------------------------------------------------------------------------------------------ */
int pca_nusc_project_cams(pca_ctx *ctx, const double *pc_lidar, int32_t n, const double T_ego_from_lidar[16],
                          const double T_glob_from_ego[16], const double *T_cam_from_glob, const double *K,
                          const double *wh, int ncam, double *pc_in_ego, double *uv, int64_t *cam_idx,
                          void *stream);

/* ------------------------------------------------------------------------------------------------
 * K0s NuScenes sweep merging + GT-box point labelling: the lidar sweeps of one sample into the keyframe's lidar frame,
 *     points next to the sensor axis dropped, every point labelled with the track index and class of the LAST candidate
 *     box of its own sweep that contains it.  Replaces the per-point part of inst_centric_get_sweeps,
 *     datasets/nuscenes_utils.py:233-243, :312-329, :332-531 (the dataset walk and the per-track lists stay on the host).
 *     raw: dev f32 [n_points][5], the sweeps' .bin rows concatenated oldest sweep first (column 4 is never read).
 *     sweeps / boxes: HOST tables (they travel through the context's pinned block, fetched by a kernel); a sweep's boxes
 *       are consecutive.  Limits: PCA_NUSC_MAX_SWEEPS sweeps, PCA_NUSC_MAX_SWEEP_BOXES boxes, PCA_NUSC_MAX_SWEEP_TILES tiles
 *       of 512 points (a tile never straddles a sweep; every sweep has at least one); beyond them -1, the limit named by
 *       pca_last_error, nothing launched.
 *     Per point: keep = sqrt(x*x + y*y) > center_radius in un-fused f32; xyz' = f32(T . [x y z 1]) (f64 fma chain in k
 *       order); per box: local = inv . [xyz' 1] (the same chain over the f32-rounded xyz'), inside iff
 *       fabs(local[a] / size[a]) < inside_limit on the three axes (IEEE f64 division; NaN, inf, size 0: false).
 *     points_out: dev f32 [<= n_points][8] rows x', y', z', intensity, lag, sweep, inst, cls of the kept points, in sweep
 *       order then point order; inst = index of the box's track (a box opens a track iff it has a hit and no earlier box
 *       of the same track_key has; tracks are numbered in box order), cls = the box's class, both -1 without a box.
 *     tally_out: dev int32 [n_sweeps + 1 + n_boxes]: the kept rows before every sweep (and their total), then per box
 *       the number of kept points of its sweep inside it.
 *     workspace: dev, pca_nusc_merge_sweeps_workspace_bytes(n_points, n_boxes) bytes.  Two launches, no synchronisation.
 *     PCA_NUSC_SWEEPS_PRETEST=0 turns the certified comparison that spares most divisions off (A/B; same results).
 * ------------------------------------------------------------------------------------------------ */
#define PCA_NUSC_MAX_SWEEPS 32
#define PCA_NUSC_MAX_SWEEP_BOXES 4096
#define PCA_NUSC_MAX_SWEEP_TILES 16384
typedef struct {
    int32_t row0, n_rows;      /* the sweep's rows of raw */
    int32_t box0, n_boxes;     /* its candidate boxes */
    float lag, sweep;          /* columns 4, 5 of its points */
    double T[12];              /* rows 0..2 of target_from_sweep */
} pca_nusc_sweep;
typedef struct {
    double inv[12];            /* rows 0..2 of inv(target_from_box) */
    double size[3];            /* l, w, h */
    int32_t cls;               /* class index */
    int32_t track_key;         /* ordinal of the box's instance token among the call's candidates, 0 .. n_boxes - 1 */
} pca_nusc_sweep_box;
int64_t pca_nusc_merge_sweeps_workspace_bytes(int64_t n_points, int n_boxes);
int pca_nusc_merge_sweeps(pca_ctx *ctx, const float *raw /*dev*/, int64_t n_points, const pca_nusc_sweep *sweeps,
                          int n_sweeps, const pca_nusc_sweep_box *boxes, int n_boxes, float center_radius,
                          double inside_limit, void *workspace /*dev*/, int64_t workspace_bytes,
                          float *points_out /*dev*/, int32_t *tally_out /*dev*/, void *stream);

/* ------------------------------------------------------------------------------------------------
 * K2  in-place rigid re-transform of every stored point of frames [slot_begin, slot_end).
 *     Replaces sem_pc_accum.py:167-183 (update_sem_pcs).  Ts: n_T 4x4 row-major matrices applied one
 *     after the other (n_T = 1 is the reference's per-step call; n_T > 1 applies a backlog of steps in
 *     one pass over HBM per 16 transforms, with identical roundings).  0 <= n_T <= 65535 (more: -1, nothing launched).
 * ------------------------------------------------------------------------------------------------ */
int pca_retransform(pca_ctx *ctx, const pca_store *store, const int64_t *frame_off /*dev*/, int slot_begin,
                    int slot_end, const double *Ts, int n_T, void *stream);

/* Batched integrate: k frames appended by ONE K1 call into slots first_slot .. first_slot+k-1, with the per-frame
 * transforms Ts[0..k) (Ts[i] = T_new_prev of frame i).  Frame i still owes Ts[i+1] .. Ts[k-1] (the reference applies
 * them one integrate() at a time, sem_pc_accum.py:167-183); this applies them, frame by frame, in ceil((k-1)/16)
 * launches with the roundings of the step-by-step form.  (Frames stored BEFORE the batch owe all k: pca_retransform.) */
int pca_retransform_batch_tail(pca_ctx *ctx, const pca_store *store, const int64_t *frame_off /*dev*/, int first_slot,
                               int n_frames, const double *Ts, void *stream);

/* ------------------------------------------------------------------------------------------------
 * K3  dyn[p] = 1 where inst[p] == inst_idx, for n_pairs (slot, inst_idx) pairs.
 *     Replaces nuscenes_oracle_sem_pc_accum.py:223-229, :243-250.
 * ------------------------------------------------------------------------------------------------ */
int pca_mark_dynamic(pca_ctx *ctx, const pca_store *store, const int64_t *frame_off /*dev*/, const int32_t *slots,
                     const int32_t *inst_idx, int n_pairs, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Voxel de-duplication of the accumulation buffer (opt-in; no reference counterpart -- the reference only
 *     evicts whole frames by horizon, sem_pc_accum.py:185-209).  Over the stored points of frames
 *     [slot_begin, slot_end): of all points in one voxel floor(xyz / voxel_size) the first in store order (the
 *     oldest observation) stays.  Segments are compacted in place, order-preserving; frame_off[slot_begin+1 ..
 *     slot_end] is rewritten.  slot_end must be the last used slot (later segments are not moved).
 *     The key holds 21 bits per axis: voxel indices are clamped to [-2^20, 2^20) per axis, i.e. +-2^20 * voxel_size metres
 *     (+-inf included).  Every point beyond that shares the boundary voxel of its side -- with the points that really lie in
 *     it -- and only the first of them stays.
 * ------------------------------------------------------------------------------------------------ */
int64_t pca_voxel_dedup_workspace_bytes(int64_t max_points, int n_slots);
int pca_voxel_dedup(pca_ctx *ctx, const pca_store *store, int64_t *frame_off /*dev*/, int slot_begin, int slot_end,
                    double voxel_size, int64_t max_points, void *workspace /*dev*/, int64_t workspace_bytes,
                    void *stream);

/* ------------------------------------------------------------------------------------------------
 * Point-to-plane ICP between two lidar sweeps.  Replaces the Open3D calls
 *       sem_pc_accum.py:310-315 (estimate_normals, default 30 nearest neighbours) and
 *       kitti360_sem_pc_accum.py:115-127 (registration_icp(source = previous sweep, target = new sweep, threshold,
 *       init, PointToPlane), defaults: <= 30 iterations, relative fitness / rmse 1e-6).
 *     Open3D is a third-party, unpinned dependency of the reference: parity is UNPINNED; the tests check known
 *     motions and a k-d-tree CPU model of this algorithm.  Neighbour searches are exact inside a cap (normals 3 m,
 *     correspondences min(max_corr_dist, 4 m)); sweeps must lie within +-128 m (x, y), -16..16 m (z) of the sensor.
 *     src_pts / tgt_pts: dev [n,4] f32 rows x,y,z,(ignored).  init / T_out: host 4x4 row-major; T_out maps source
 *     coordinates into the target frame (T_new_prev).  Synchronises `stream` before returning.
 *     max_iter < 1 means 30; max_iter above PCA_ICP_MAX_ITER is refused before anything is launched ("icp: max_iter must not
 *     exceed 32766").  A registration that no convergence test ends takes exactly max_iter updates: *iterations == max_iter.
 * ------------------------------------------------------------------------------------------------ */
#define PCA_ICP_MAX_ITER 32766
int64_t pca_icp_workspace_bytes(int32_t max_points);   /* max_points >= max(n_src, n_tgt) */
int pca_icp_register(pca_ctx *ctx, const float *src_pts /*dev*/, int32_t n_src, const float *tgt_pts /*dev*/,
                     int32_t n_tgt, double max_corr_dist, const double init[16], int max_iter, double rel_fitness,
                     double rel_rmse, void *workspace /*dev*/, int64_t workspace_bytes, double T_out[16],
                     double *fitness, double *rmse, int *iterations, void *stream);

/* ------------------------------------------------------------------------------------------------
 * K4-K7  BEV rasteriser: window [slot_begin, slot_end), 'present' = [slot_begin, slot_split),
 *     'future' = [slot_split, slot_end), 'full' = both.  Replaces
 *       kitti360_sem_pc_accum.py:189-213 / nuscenes_oracle_sem_pc_accum.py:535-581 (window assembly, origin),
 *       bev_generator/bev_generator.py:127-160, :207-255, :737-747 (rotate, translate, crop, height, floor),
 *       bev_generator/sem_bev.py:57-118 (static partition, maps), :535-554 (min z), :619-669 (rgb median),
 *       bev_generator/bev_generator.py:373-480 (counts, dirichlet, intensity), sem_bev.py:593-617, :204-257 (fp16).
 *     Output (dev): planes f64 [21,px,px] and/or planes_f16 [21,px,px] (either may be NULL), order
 *       set-major {present,future,full} x {road,intensity,r,g,b,dynamic,elevation}.
 *     Grid: 1 <= px <= 4096 (else "bev: px must be in 1..4096").  Up to 1024 the grid is one piece; above, it runs as bands
 *       of whole 8-cell tile rows of at most 16 384 tiles each (2048: 4 bands, 4096: 16), one pass over the window and one
 *       launch of the tile kernels per band, all in the caller's planes -- same results as any other banding.  A banded call
 *       takes no deferred K1 along (pca_k1_defer: it runs on its own first).
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    double origin[3];         /* bev_frame_coords                                                   */
    double R[9];              /* rotation_matrix_3d(rot_ang) evaluated on the host (np.cos/np.sin);
                                 must be a rotation about z (checked)                                */
    double dx, dy;            /* augmentation translation                                           */
    double view;              /* zoom_scalar * view_size                                            */
    double height_filter;     /* keep z < height_filter; NaN disables                               */
    double int_scaler, int_sep_scaler, int_mid_threshold;
    double rgb_fill;          /* value of an empty cell before /255                                 */
    int32_t px;               /* grid side [cells], 1..4096 (> 1024: banded, see above)         */
    int32_t road_class;
    uint64_t dynobj_mask[4];  /* classes counted in the 'dynamic' plane                             */
    int32_t intensity_div255;
    int32_t pad;
} pca_bev_params;

/* bytes of scratch the rasteriser needs for a window of at most max_points and a px x px grid (px > 1024: the bands share it) */
int64_t pca_bev_workspace_bytes(int64_t max_points, int px);

/* intensity64 (dev, may be NULL): f64 intensities indexed like the store, overriding store.intensity
 * (for callers whose column 3 is not f32-representable).  max_points bounds the window size.
 * pending_T (host, 4x4 row-major, may be NULL): a re-transform that is still owed to the frames
 * [slot_begin, pending_slot_end) (sem_pc_accum.py:167-183).  It is applied -- and written back to the store,
 * exactly as pca_retransform would -- by the first kernel of the rasteriser, which reads those coordinates
 * anyway; this saves one full read of the store per step when every integrate() is followed by a BEV. */
int pca_bev_generate(pca_ctx *ctx, const pca_store *store, const double *intensity64,
                     const int64_t *frame_off /*dev*/, int slot_begin, int slot_split, int slot_end,
                     int64_t max_points, const pca_bev_params *prm, const double *pending_T, int pending_slot_end,
                     void *workspace /*dev*/, int64_t workspace_bytes, double *planes /*dev*/,
                     uint16_t *planes_f16 /*dev*/, void *stream);

/* Same rasteriser with EXTRA REDUCERS (opt-in; the reference's live code has none of them -- mean elevation /
 * mean intensity exist only in its unused legacy utils/bev_generation.py:249-294).  extra_planes: dev f64
 * [3 sets][PCA_BEV_EXTRA_PLANES][px][px], per set {max z, mean z} over the static points of a cell (0 where
 * unobserved, like the elevation plane) and {mean raw intensity} over its road points (0 where none).
 * Sums are exact fixed-point integers: the result does not depend on the order of the points. */
#define PCA_BEV_EXTRA_PLANES 3
int pca_bev_generate_ex(pca_ctx *ctx, const pca_store *store, const double *intensity64,
                        const int64_t *frame_off /*dev*/, int slot_begin, int slot_split, int slot_end,
                        int64_t max_points, const pca_bev_params *prm, const double *pending_T, int pending_slot_end,
                        void *workspace /*dev*/, int64_t workspace_bytes, double *planes /*dev*/,
                        uint16_t *planes_f16 /*dev*/, double *extra_planes /*dev, may be NULL*/, void *stream);

/* The same with a CHAIN of owed re-transforms (sem_pc_accum.py:167-183 issues one per integrate): transform k (4x4 row-major
 * in pending_Ts[16 k ..], oldest first) is owed by slots [slot_begin, pending_slot_ends[k]) (ascending).  The rasteriser
 * applies them one after the other to the coordinates it reads -- the roundings of one pca_retransform pass each -- and,
 * with write_back != 0, stores the result (the transforms are then no longer owed); with write_back == 0 they stay owed
 * and the store is untouched: the caller passes them again, together with the next one, and saves the 24 B per stored
 * point of the write-back on that call.  n_pending <= PCA_BEV_MAX_CHAIN. */
#define PCA_BEV_MAX_CHAIN 4
int pca_bev_generate_chain(pca_ctx *ctx, const pca_store *store, const double *intensity64,
                           const int64_t *frame_off /*dev*/, int slot_begin, int slot_split, int slot_end,
                           int64_t max_points, const pca_bev_params *prm, const double *pending_Ts,
                           const int *pending_slot_ends, int n_pending, int write_back, void *workspace /*dev*/,
                           int64_t workspace_bytes, double *planes /*dev*/, uint16_t *planes_f16 /*dev*/,
                           double *extra_planes /*dev, may be NULL*/, void *stream);

/* Several rasters of ONE store in one launch of each kernel: the sweep over present_idx of a finished scene
 * (run_nuscenes_bev_gen.py:245-271 walks present_idx over a store that no longer changes) or the bev_num augmented samples
 * of one window (kitti360_sem_pc_accum.py:236-241, a multiprocessing.Pool in the reference).  Each job is what one
 * pca_bev_generate call takes (slots, parameters, output planes); no owed transforms; workspace:
 * n_jobs * round_up(pca_bev_workspace_bytes(max_points, px), 256) + 256 bytes.  Results equal n_jobs single calls. */
typedef struct {
    int32_t slot_begin, slot_split, slot_end, reserved;
    pca_bev_params prm;
    double *planes;            /* dev [21,px,px] f64 or NULL */
    uint16_t *planes_f16;      /* dev [21,px,px] f16 or NULL */
} pca_bev_job;
int pca_bev_generate_many(pca_ctx *ctx, const pca_store *store, const double *intensity64 /*dev or NULL*/,
                          const int64_t *frame_off /*dev*/, const pca_bev_job *jobs, int n_jobs, int64_t max_points,
                          void *workspace /*dev*/, int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * BEV planes of ANY semantic class group, all groups counted in one pass over the window.  Replaces
 *       bev_generator/bev_generator.py:373-394 (gen_sem_probmap: partition by a list of classes, two count maps,
 *       dirichlet expectation), :417-436 (partition_semantic_pc), :438-455 (gen_gridmap_count_map), :457-480
 *       (dirichlet_dist_expectation) for the static partition of the window (sem_bev.py:57-69), and the geometry of
 *       bev_generator/bev_generator.py:127-160, :207-255, :737-747 exactly as the rasteriser above evaluates it
 *       (owed re-transforms oldest first, origin, R, dx / dy, strict crop, z < height_filter, dyn != 1, floor to the grid,
 *       clamp, image rows; a point whose z is not finite is dropped).
 *     groups[g]: the 256-bit class set of group g, laid out like pca_bev_params.dynobj_mask; groups may overlap.
 *     Per (cell, set) with n static points, n_g of them in group g:  prob = (n_g + 1) / ((n_g + 1) + ((n - n_g) + 1)).
 *     Output (dev, any of them may be NULL, not all): prob f64 / prob_f16 [3 sets][n_groups][px][px], counts u32
 *       [3 sets][n_groups + 1][px][px] (slot n_groups = all static points); set order {present, future, full}.
 *     Of prm, origin, R (a rotation about z, checked), dx, dy, view, height_filter and px are read.
 *     Grid: 1 <= px <= 1024 (else "bev class planes: px must be in 1..1024": no banding); 1 <= n_groups <= 16.
 *     The store is never written: owed re-transforms (pending_Ts / pending_slot_ends / n_pending as pca_bev_generate_chain
 *     takes them) are applied to what is read and stay owed.  A K1 noted by pca_k1_defer runs on its own first; a bin range
 *     armed by pca_bev_bin_range / pca_bev_view_hint is neither used nor cleared (the whole window is read).  A window above
 *     max_points is cut there and raises PCA_STATUS_STORE_OVERFLOW; a window without points gives prob 0.5 and counts 0.
 *     Every argument is checked before anything is launched; -1 with pca_last_error set.
 * ------------------------------------------------------------------------------------------------ */
#define PCA_BEV_MAX_CLASS_GROUPS 16
typedef struct { uint64_t mask[4]; } pca_class_group;      /* 256-bit class set, laid out like dynobj_mask */
int64_t pca_bev_class_workspace_bytes(int64_t max_points, int px);
int pca_bev_class_planes(pca_ctx *ctx, const pca_store *store, const int64_t *frame_off /*dev*/,
                         int slot_begin, int slot_split, int slot_end, int64_t max_points,
                         const pca_bev_params *prm,
                         const pca_class_group *groups, int n_groups,
                         const double *pending_Ts, const int *pending_slot_ends, int n_pending,
                         void *workspace /*dev*/, int64_t workspace_bytes,
                         double *prob      /*dev [3][n_groups][px][px]   or NULL*/,
                         uint16_t *prob_f16/*dev, same shape             or NULL*/,
                         uint32_t *counts  /*dev [3][n_groups+1][px][px] or NULL; slot n_groups = all static points*/,
                         void *stream);

/* ------------------------------------------------------------------------------------------------
 * The BEV window partitioned by height above the cell minimum.  Replaces
 *       bev_generator/sem_bev.py:556-591 (static_obj_partitioning_by_elev: the per-cell minimum-z map of the rows it is
 *       given, then every row whose z lies more than elev_thresh above its cell's minimum is flagged; two per-point Python
 *       loops), and the geometry of bev_generator/bev_generator.py:127-160, :207-255, :737-747 exactly as the rasteriser
 *       above evaluates it (owed re-transforms oldest first, origin, R, dx / dy, strict crop, z < height_filter, floor to
 *       the grid, clamp, image rows; a point whose z is not finite is dropped).
 *     include_dyn == 0: points with dyn == 1 are dropped (the static partition generate_bev uses, sem_bev.py:57-69);
 *       include_dyn != 0: they take part (the reference's method never looks at dyn).
 *     A point's z is (Z - origin z) + 0.0 in f64: -0.0 arrives as +0.0, as the reference's np.matmul delivers it.
 *     elevated = z > (min z of the cell + elev_thresh): an f64 add and a strict f64 compare.  elev_thresh may be negative
 *       (the reference accepts it); NaN is refused.
 *     Output (dev, any of them may be NULL, not all): elev f64 [px][px] (the cell minimum, 0.0 where no point), observed u8
 *       [px][px] (0 / 1), flags u8 [window points] in window order (0 kept, 1 elevated, 255 not in view; every byte of the
 *       window is written exactly once, the caller need not clear it), counts int64 [3] {in view, elevated, not elevated}.
 *     Of prm, origin, R (a rotation about z, checked), dx, dy, view, height_filter and px are read.
 *     Grid: 1 <= px <= 1024 (else "bev elev partition: px must be in 1..1024": no banding).
 *     The store is never written: owed re-transforms (pending_Ts / pending_slot_ends / n_pending as pca_bev_generate_chain
 *     takes them) are applied to what is read and stay owed.  A K1 noted by pca_k1_defer runs on its own first; a bin range
 *     armed by pca_bev_bin_range / pca_bev_view_hint is neither used nor cleared (the whole window is read).  A window above
 *     max_points is cut there and raises PCA_STATUS_STORE_OVERFLOW (flags beyond the cut are not written); a window without
 *     points gives elev 0, observed 0 and counts 0.  The window index must fit 32 bits.
 *     Every argument is checked before anything is launched; -1 with pca_last_error set.
 * ------------------------------------------------------------------------------------------------ */
int64_t pca_bev_elev_workspace_bytes(int64_t max_points, int px);
int pca_bev_elev_partition(pca_ctx *ctx, const pca_store *store, const int64_t *frame_off /*dev*/,
                           int slot_begin, int slot_end, int64_t max_points,
                           const pca_bev_params *prm, double elev_thresh, int include_dyn,
                           const double *pending_Ts, const int *pending_slot_ends, int n_pending,
                           void *workspace /*dev*/, int64_t workspace_bytes,
                           double *elev      /*dev [px][px]         or NULL*/,
                           uint8_t *observed /*dev [px][px]         or NULL*/,
                           uint8_t *flags    /*dev [window points]  or NULL: 0 kept, 1 elevated, 255 not in view*/,
                           int64_t *counts   /*dev [3]: in view, elevated, not elevated; or NULL*/,
                           void *stream);

/* ------------------------------------------------------------------------------------------------
 * The BEV window voxelised into semantic occupancy labels: the grid with a height axis, a majority vote per voxel (what
 *       SemanticKITTI-SSC / SSCBench-KITTI-360 labels are made from).  No reference counterpart: an extension on the
 *       scaffold of the two passes above.  The geometry is that of pca_bev_elev_partition (owed re-transforms oldest first,
 *       origin, R, dx / dy, strict crop, z < height_filter, floor to the grid, clamp, image rows; a point whose z is not
 *       finite is dropped).
 *     include_dyn == 0: points with dyn == 1 are dropped; include_dyn != 0: they take part.
 *     label_of (host, 256 bytes): the label of a kept point is label_of[its class byte]; 255: the point takes no part;
 *       any other value must be < n_labels.  Several classes may share a label.
 *     Height bin: z = (Z - origin z) + 0.0, t = (z - z_lo) / z_step, k = floor(t), all f64, the division IEEE.  A point
 *       is kept iff 0 <= k < nz: in z NOTHING is clamped, a point below z_lo or at or above z_lo + nz z_step is dropped.
 *     Per voxel (k, row, col) with n_l kept points of label l:  counts = sum n_l,  top = max n_l,  labels = the smallest l
 *       with n_l == top, 255 where counts == 0.  The counters are 32 bits wide.
 *     Output (dev, any of them may be NULL, not all): labels u8, counts u32, top u32, each [nz][px][px].
 *     Scope: an EMPTY voxel is one no kept point fell into.  Whether it is free space or merely unseen is not decided
 *       here: pca_bev_voxel_rays (below) casts the rays and tells the two apart.
 *     Of prm, origin, R (a rotation about z, checked), dx, dy, view, height_filter and px are read.
 *     Limits: 1 <= px <= 1024 (else "bev voxel labels: px must be in 1..1024": no banding), 1 <= nz <= 32,
 *       1 <= n_labels <= 32; z_lo finite; z_step finite and > 0.
 *     The store is never written: owed re-transforms (pending_Ts / pending_slot_ends / n_pending as pca_bev_generate_chain
 *     takes them) are applied to what is read and stay owed.  A K1 noted by pca_k1_defer runs on its own first; a bin range
 *     armed by pca_bev_bin_range / pca_bev_view_hint is neither used nor cleared (the whole window is read).  A window above
 *     max_points is cut there and raises PCA_STATUS_STORE_OVERFLOW; a window without points gives labels 255, counts 0 and
 *     top 0.  Every argument is checked before anything is launched; -1 with pca_last_error set.
 * ------------------------------------------------------------------------------------------------ */
#define PCA_BEV_VOXEL_MAX_Z 32
#define PCA_BEV_VOXEL_MAX_LABELS 32
int64_t pca_bev_voxel_workspace_bytes(int64_t max_points, int px);
int pca_bev_voxel_labels(pca_ctx *ctx, const pca_store *store, const int64_t *frame_off /*dev*/,
                         int slot_begin, int slot_end, int64_t max_points,
                         const pca_bev_params *prm, double z_lo, double z_step, int nz,
                         const uint8_t label_of[256] /*host*/, int n_labels, int include_dyn,
                         const double *pending_Ts, const int *pending_slot_ends, int n_pending,
                         void *workspace /*dev*/, int64_t workspace_bytes,
                         uint8_t  *labels /*dev [nz][px][px] or NULL*/,
                         uint32_t *counts /*dev [nz][px][px] or NULL*/,
                         uint32_t *top    /*dev [nz][px][px] or NULL*/,
                         void *stream);

/* ------------------------------------------------------------------------------------------------
 * Lidar rays cast through the voxel grid of pca_bev_voxel_labels: which voxels a beam crossed on its way from the sensor to
 *       a stored point.  With the labels' counts: occupied (counts > 0), else free (seen), else unseen -- the "invalid" mask
 *       of SemanticKITTI-SSC / SSCBench-KITTI-360 ground truth.  No reference counterpart.  One ray per stored point of the
 *       window, from the sensor position of its slot (origins, one per slot, in the store's CURRENT coordinates: the pose
 *       track; they owe nothing) to the point (owed re-transforms applied, oldest first).
 *     Everything is f64, each operation rounded on its own, nothing fused; the product sum is deliberately UNFUSED (unlike
 *       the view test of the passes above), the divisions are IEEE.  Grid coordinates of a position (X, Y, Z):
 *         x = X - ox, y = Y - oy;  ax = (r0 x + r1 y) + dx,  ay = (r3 x + r4 y) + dy;
 *         u = ax / view * px + 0.5 px,  v = ay / view * px + 0.5 px,  w = (((Z - oz) + 0.0) - z_lo) / z_step.
 *       Its voxel is (i, j, k) = (floor u, floor v, floor w), unclamped; inside the grid iff 0 <= i, j < px and 0 <= k < nz;
 *       its place in the output is [k][px - 1 - j][i] (image rows).
 *     Every point of the window casts a ray, except a point with dyn == 1 when include_dyn == 0.  The crop, height_filter
 *       and the class play no part: a beam to a point outside the view or above the filter still crossed the grid.
 *     A ray whose start or end has a grid coordinate that is not finite or is >= 2^30 in magnitude is dropped (stats[2]).
 *       With start voxel c, end voxel g and n_a = |g_a - c_a|, a ray whose N = n_0 + n_1 + n_2 exceeds
 *       PCA_BEV_RAYS_MAX_STEPS is dropped (stats[3]): the cap is a condition, it bounds every launch.
 *     Traversal (Amanatides-Woo, driven by the integer step counts, so that it always ends in the end voxel), axes in the
 *       order (u, v, w): d_a = e_a - s_a, step_a = sign(g_a - c_a); for n_a > 0: tMax_a = ((c_a + (step_a > 0 ? 1 : 0)) -
 *       s_a) / d_a, tDelta_a = 1 / |d_a|, else tMax_a = +inf.  N times: mark the current voxel if it is inside the grid;
 *       a = 0 if t0 <= t1 && t0 <= t2, else 1 if t1 <= t2, else 2; c_a += step_a, n_a -= 1; tMax_a = n_a ? tMax_a +
 *       tDelta_a : +inf.  The end voxel is never marked by its own ray; a ray with N = 0 marks nothing.
 *     Output (dev, either may be NULL, not both; both are cleared by the call itself, on the stream):
 *       seen u8 [nz][px][px]: 1 = at least one ray passed through, else 0;
 *       stats i64 [4]: points considered, rays cast (not dropped), dropped not finite, dropped too long.
 *     Scope: ONE origin per stored frame (the merged sweeps of a NuScenes sample share their key frame's origin); no
 *       per-beam minimum or maximum range.
 *     Of prm, origin, R (a rotation about z, checked), dx, dy, view and px are read.
 *     Limits: 1 <= px <= 1024 (else "bev voxel rays: px must be in 1..1024"), 1 <= nz <= 32; z_lo finite; z_step finite
 *       and > 0; slot_begin <= slot_end.  No workspace.
 *     The store is never written: owed re-transforms (pending_Ts / pending_slot_ends / n_pending as pca_bev_generate_chain
 *     takes them) are applied to the points that are read and stay owed.  A K1 noted by pca_k1_defer runs on its own first; a
 *     bin range armed by pca_bev_bin_range / pca_bev_view_hint is neither used nor cleared.  A window above max_points is
 *     cut there and raises PCA_STATUS_STORE_OVERFLOW; a window without points gives all zeros.  Every argument is checked
 *     before anything is launched; -1 with pca_last_error set.
 * ------------------------------------------------------------------------------------------------ */
#define PCA_BEV_RAYS_MAX_STEPS 16384
int pca_bev_voxel_rays(pca_ctx *ctx, const pca_store *store, const int64_t *frame_off /*dev*/,
                       int slot_begin, int slot_end, int64_t max_points,
                       const pca_bev_params *prm, double z_lo, double z_step, int nz, int include_dyn,
                       const double *origins /*dev [slot_end - slot_begin][3]: sensor position of each slot, store coordinates, current (nothing owed)*/,
                       const double *pending_Ts, const int *pending_slot_ends, int n_pending,
                       uint8_t *seen  /*dev [nz][px][px]: 1 = at least one ray passed through, else 0; or NULL*/,
                       int64_t *stats /*dev [4]: points considered, rays cast, dropped not finite, dropped too long; or NULL*/,
                       void *stream);

/* ------------------------------------------------------------------------------------------------
 * Free-space carving by ray hit / miss: the counting form of pca_bev_voxel_rays.  A voxel that held points of a movable
 *       class at one moment, and that the beams of other frames later passed straight through, held a moving object; its
 *       points are flagged.  No reference counterpart.  What KITTI needs, where no instance labels exist and dyn is 0 for
 *       every point, and a second opinion for the classes the NuScenes tracker does not follow.
 *     Geometry, ray set-up, drop rules, traversal order and tie order are word for word those of pca_bev_voxel_rays (f64,
 *       nothing fused, the unfused product sum, IEEE divisions; a ray with a coordinate that is not finite or >= 2^30 in
 *       magnitude is dropped, so is one over PCA_BEV_RAYS_MAX_STEPS; Amanatides-Woo driven by the integer step counts, axes
 *       in the order (u, v, w); the place of voxel (i, j, k) in the output is [k][px - 1 - j][i]).
 *     A point TAKES PART iff it lies inside the window cut at max_points and (include_dyn != 0 or dyn != 1).  Every point that
 *       takes part has a ray from its slot's origin to itself; if that ray is not dropped it is CAST.
 *     hits[v]: the number of cast rays whose end voxel is v and lies inside the grid.  The class, the crop and height_filter
 *       play no part, as in the rays pass.
 *     A CANDIDATE POINT is a point with a cast ray, an end voxel inside the grid and a class in `only`; a CANDIDATE VOXEL holds
 *       at least one candidate point.
 *     cross[v], for a candidate voxel: the number of cast rays that have a traversal step `it` (0-based, of N) with
 *       it < N - end_margin at voxel v.  A ray visits a voxel at most once, and its end voxel is never counted by itself.
 *       cross[v] is 0 for every voxel that is NOT a candidate voxel (the kernel counts only where it has to).
 *     A candidate point in voxel v is FLAGGED iff cross[v] >= min_cross and (double)cross[v] >= ratio * (double)hits[v]: one
 *       f64 multiply and one compare.
 *     Output (dev, any of them may be NULL, not all; hits, cross and stats are cleared by the call itself, on the stream):
 *       hits, cross u32 [nz][px][px]; flags u8 [window points] in window order: 1 flagged, 0 candidate kept, 255 everything
 *       else (every byte of the cut window is written exactly once, bytes beyond the cut are not written);
 *       stats i64 [6]: points that take part, rays cast, dropped not finite, dropped too long, candidate points, flagged
 *       points.  All sums are integer sums: the result does not depend on the order of the points.
 *     Scope: ONE origin per stored frame; the rays of a point's own frame count like any other -- end_margin is what keeps a
 *       surface from carving itself (neighbouring beams of one surface cross its voxels just before they end), and ratio is
 *       what keeps a surface that is hit as often as it is crossed; no automatic call from integrate().
 *     Of prm, origin, R (a rotation about z, checked), dx, dy, view and px are read.
 *     Limits: 1 <= px <= 1024, 1 <= nz <= 32; z_lo finite; z_step finite and > 0; 0 <= end_margin <= PCA_BEV_RAYS_MAX_STEPS;
 *       min_cross >= 1; ratio finite and >= 0; origins and only not NULL; workspace of pca_bev_carve_workspace_bytes(max_points,
 *       px, nz) bytes; max_points < 2^32; slot_begin <= slot_end.
 *     The store is never written: owed re-transforms (pending_Ts / pending_slot_ends / n_pending as pca_bev_generate_chain
 *     takes them) are applied to the points that are read and stay owed.  A K1 noted by pca_k1_defer runs on its own first; a
 *     bin range armed by pca_bev_bin_range / pca_bev_view_hint is neither used nor cleared.  A window above max_points is
 *     cut there and raises PCA_STATUS_STORE_OVERFLOW; a window without points gives all zeros and writes no flags.  Every
 *     argument is checked before anything is launched; -1 with pca_last_error set ("bev voxel carve: ..."), nothing written.
 * ------------------------------------------------------------------------------------------------ */
int64_t pca_bev_carve_workspace_bytes(int64_t max_points, int px, int nz);
int pca_bev_voxel_carve(pca_ctx *ctx, const pca_store *store, const int64_t *frame_off /*dev*/,
                        int slot_begin, int slot_end, int64_t max_points,
                        const pca_bev_params *prm, double z_lo, double z_step, int nz, int include_dyn,
                        const double *origins /*dev [slot_end - slot_begin][3]: sensor position of each slot, as pca_bev_voxel_rays takes them*/,
                        const pca_class_group *only /*the classes that may be flagged; not NULL*/,
                        int end_margin, uint32_t min_cross, double ratio,
                        const double *pending_Ts, const int *pending_slot_ends, int n_pending,
                        void *workspace /*dev*/, int64_t workspace_bytes,
                        uint32_t *hits  /*dev [nz][px][px] or NULL*/,
                        uint32_t *cross /*dev [nz][px][px] or NULL*/,
                        uint8_t  *flags /*dev [window points] or NULL: 1 flagged, 0 candidate kept, 255 everything else*/,
                        int64_t  *stats /*dev [6] or NULL*/,
                        void *stream);

/* ------------------------------------------------------------------------------------------------
 * The object voxels of the window clustered into instances: Euclidean clustering on the voxel grid of pca_bev_voxel_labels,
 *       that is connected-component labelling of its occupied voxels, a deterministic numbering of the components, and the
 *       instance of every stored point.  No reference counterpart.  What KITTI needs to say which points form one object
 *       (panoptic occupancy ground truth, per-object boxes and counts, a carved mover treated as one thing).
 *     Geometry and kept points are word for word those of pca_bev_voxel_labels, from the same code: owed re-transforms
 *       oldest first, origin, R about z, dx / dy, strict crop, z < height_filter, floor, clamp, image rows; the f64 height
 *       bin with the IEEE division, nothing clamped in z; a point whose label_of[class] is 255 takes no part.  counts[v]
 *       below IS pca_bev_voxel_labels' counts for the same label table and the same dyn rule.
 *     dyn_mode 0: points with dyn == 1 take no part; 1: every point takes part; 2: ONLY points with dyn == 1 take part (the
 *       movers after a carve that marked them, or of a NuScenes window).
 *     Foreground: voxel v is foreground iff counts[v] >= min_points (min_points >= 1).
 *     Neighbours, on the output index (k, row, col), place = (k px + row) px + col: connectivity 6 -- exactly one coordinate
 *       differs, by 1; connectivity 26 -- no coordinate differs by more than 1 and not all are equal.  Nothing wraps:
 *       (k, row, px - 1) and (k, row + 1, 0) are adjacent places and NOT neighbours, nor are the last row of a height plane
 *       and the first row of the next.
 *     A component is a maximal connected set of foreground voxels; its root is its smallest place; it SURVIVES iff it has at
 *       least min_voxels voxels (min_voxels >= 1).  The n surviving components are numbered 0 .. n - 1 in ascending order
 *       of their roots: the numbering is a function of the kept points as a set, not of their order or of any scheduling.
 *     Output (dev, any of them may be NULL, not all; each is cleared or fully written by the call itself, on the stream):
 *       inst i32 [nz][px][px]: the id of the surviving component that holds the voxel, else -1;
 *       ids i32 [window points], window order: inst of the voxel of a kept point, -1 for every other point (every entry of the
 *         cut window is written exactly once, nothing behind the cut is written); neither inst nor ids is capped by
 *         max_instances;
 *       table u32 [max_instances][PCA_BEV_INST_COLS], row id < min(n, max_instances): root place, voxels, kept points,
 *         col_min, col_max, row_min, row_max, k_min, k_max; the rows from n on are zero;
 *       label_counts u32 [max_instances][n_labels]: the kept points of label l in instance id;
 *       stats i64 [6]: kept points, foreground voxels, components, surviving components (n), kept points with ids >= 0,
 *         voxels of the largest surviving component.
 *       All sums are integer sums and all extremes integer extremes: exact and free of any order.
 *     Scope: the boxes are VOXEL boxes (pca_amd.host_logic.instance_boxes turns the voxel box into metres); the metric box
 *       tighter than the voxels is pca_bev_instance_boxes', from this call's ids.  No automatic call from integrate().
 *     Of prm, origin, R (a rotation about z, checked), dx, dy, view, height_filter and px are read.
 *     Limits: 1 <= px <= 1024, 1 <= nz <= 32, 1 <= n_labels <= 32, connectivity 6 or 26, 1 <= max_instances <= 65536,
 *       max_points < 2^31, z_lo finite, z_step finite and > 0, dyn_mode 0..2, min_points >= 1, min_voxels >= 1, a workspace
 *       of pca_bev_instances_workspace_bytes(max_points, px, nz, max_instances) bytes.
 *     The call enqueues a fixed number of launches and never waits for the device; no kernel waits for another workgroup.
 *     The store is never written: owed re-transforms (pending_Ts / pending_slot_ends / n_pending as pca_bev_generate_chain
 *     takes them) are applied to the points that are read and stay owed.  A K1 noted by pca_k1_defer runs on its own first; a
 *     bin range armed by pca_bev_bin_range / pca_bev_view_hint is neither used nor cleared.  A window above max_points is
 *     cut there and raises PCA_STATUS_STORE_OVERFLOW; a window without points gives inst -1, stats 0, zero tables and writes
 *     no ids.  Every argument is checked before anything is launched; -1 with pca_last_error set ("bev voxel instances:
 *     ..."), nothing written.
 * ------------------------------------------------------------------------------------------------ */
#define PCA_BEV_INST_COLS 9
int64_t pca_bev_instances_workspace_bytes(int64_t max_points, int px, int nz, int max_instances);
int pca_bev_voxel_instances(pca_ctx *ctx, const pca_store *store, const int64_t *frame_off /*dev*/,
                            int slot_begin, int slot_end, int64_t max_points,
                            const pca_bev_params *prm, double z_lo, double z_step, int nz,
                            const uint8_t label_of[256] /*host*/, int n_labels, int dyn_mode,
                            int min_points, int connectivity, int min_voxels, int max_instances,
                            const double *pending_Ts, const int *pending_slot_ends, int n_pending,
                            void *workspace /*dev*/, int64_t workspace_bytes,
                            int32_t  *inst         /*dev [nz][px][px] or NULL*/,
                            int32_t  *ids          /*dev [window points] or NULL*/,
                            uint32_t *table        /*dev [max_instances][PCA_BEV_INST_COLS] or NULL*/,
                            uint32_t *label_counts /*dev [max_instances][n_labels] or NULL*/,
                            int64_t  *stats        /*dev [6] or NULL*/,
                            void *stream);

/* ------------------------------------------------------------------------------------------------
 * Oriented metric boxes around the window's instances: for every instance id, the rectangle around the instance's points in
 *       each direction of a caller-given table, and the direction chosen by one of two criteria -- the search-based rectangle
 *       fit commonly used for lidar L-shapes.  No reference counterpart.  What turns "these points form one object"
 *       (pca_bev_voxel_instances) into a box tighter than the voxels: auto-labelled 3D boxes from accumulated lidar.
 *     ids: dev i32, one per window point, in window order -- what pca_bev_voxel_instances writes for the same window, but
 *       only an input here: any i32 array is legal.  A point TAKES PART iff it lies inside the window cut at max_points and
 *       0 <= ids[p] < n_rows.  Nothing else is tested (class, dyn, crop and height were tested when ids was made).
 *     cos_sin: HOST f64 [n_angles][2], (c, s) of direction t; the caller makes the table, so no libm of this library enters
 *       the result (pca_amd.host_logic.fit_angles: numpy's cos and sin of t (pi / 2) / n_angles).
 *     Coordinates, all f64 (the library is built with -ffp-contract=off: only the explicit fma fuses).  Owed re-transforms
 *       are applied oldest first, then x = X - ox, y = Y - oy, ax = fma(r1, y, r0 x) + dx, ay = fma(r4, y, r3 x) + dy -- the
 *       view test's own expressions: a point's box coordinates are the ones its cell came from -- and z = (Z - oz) + 0.0.
 *       For direction t, every operation rounded on its own: e1 = (c ax + s ay) + 0.0, e2 = (c ay - s ax) + 0.0.
 *     Per (id, t): lo1, hi1, lo2, hi2 = the extremes of e1 and e2 over the instance's points; zlo, zhi those of z; n the
 *       point count; area_t = (hi1 - lo1) (hi2 - lo2); near_t = the number of the instance's points with
 *       min(min(e1 - lo1, hi1 - e1), min(e2 - lo2, hi2 - e2)) <= edge_dist, computed iff criterion == 1 or `near` is asked
 *       for.  (A comparison with a NaN is false: a NaN is never an extreme and never near; an area_t that is NaN ranks as
 *       +inf in the choice.  ids made by pca_bev_voxel_instances name points with finite coordinates only.)
 *     t*: criterion 0 -- the smallest area_t, of equal ones the smallest t; criterion 1 -- the largest near_t, of equal ones
 *       the smaller area_t, then the smallest t (the integer form of the "closeness" criterion: it keeps an L seen from two
 *       sides from being boxed diagonally).
 *     Output (dev, any of them may be NULL, not all; each is fully written by the call itself, on the stream):
 *       fit f64 [n_rows][8]: lo1, hi1, lo2, hi2 at t*, zlo, zhi, area_t*, (double)t*; a row without a point: seven NaNs, -1;
 *       fit_n u32 [n_rows][2]: n and near_t* (0 where near was not computed);
 *       extents f64 [n_rows][n_angles][4]: lo1, hi1, lo2, hi2; a row without a point: +inf, -inf, +inf, -inf;
 *       near u32 [n_rows][n_angles];
 *       stats i64 [4]: points that take part, points with ids >= n_rows (skipped, not an error), rows with at least one
 *         point, points of the largest row.
 *       Only extremes and integer sums occur: the result is a function of the SET of (id, coordinates) pairs, not of their
 *       order or of any scheduling.
 *     Scope: the boxes stand on the ground plane (no tilt); this call tracks nothing across samples (pca_voxel_instance_match gives the ids), no instance is merged or
 *       split, the variance criterion is not offered (its float sums would depend on the order) and no KITTI label_2 /
 *       NuScenes file is written.  No automatic call from integrate().
 *     Of prm, origin, R (a rotation about z, checked), dx and dy are read.
 *     Limits: 1 <= n_rows <= 65536, 1 <= n_angles <= 256, every table entry finite, criterion 0 or 1, edge_dist finite and
 *       >= 0, max_points < 2^31, a workspace of pca_bev_instance_boxes_workspace_bytes(max_points, n_rows, n_angles) bytes
 *       (-1 outside these limits).
 *     The call enqueues a fixed number of launches whatever the data (the near kernel iff near_t is needed) and never waits
 *     for the device; no kernel waits for another workgroup.  The store is never written: owed re-transforms are applied to
 *     the points that are read and stay owed.  A K1 noted by pca_k1_defer runs on its own first; a bin range armed by
 *     pca_bev_bin_range / pca_bev_view_hint is neither used nor cleared.  A window above max_points is cut there and raises
 *     PCA_STATUS_STORE_OVERFLOW; a window without points gives empty rows and zero stats.  Every argument is checked before
 *     anything is launched; -1 with pca_last_error set ("bev instance boxes: ..."), nothing written.
 * ------------------------------------------------------------------------------------------------ */
int64_t pca_bev_instance_boxes_workspace_bytes(int64_t max_points, int n_rows, int n_angles);
int pca_bev_instance_boxes(pca_ctx *ctx, const pca_store *store, const int64_t *frame_off /*dev*/,
                           int slot_begin, int slot_end, int64_t max_points,
                           const pca_bev_params *prm,
                           const int32_t *ids     /*dev [window points]*/, int n_rows,
                           const double *cos_sin  /*host [n_angles][2]*/, int n_angles, int criterion, double edge_dist,
                           const double *pending_Ts, const int *pending_slot_ends, int n_pending,
                           void *workspace /*dev*/, int64_t workspace_bytes,
                           double   *fit     /*dev [n_rows][8] or NULL*/,
                           uint32_t *fit_n   /*dev [n_rows][2] or NULL*/,
                           double   *extents /*dev [n_rows][n_angles][4] or NULL*/,
                           uint32_t *near    /*dev [n_rows][n_angles] or NULL*/,
                           int64_t  *stats   /*dev [4] or NULL*/,
                           void *stream);

/* ------------------------------------------------------------------------------------------------
 * The window of the store rendered into a pinhole camera with a z-buffer: dense depth, colour and class targets for an
 *       image (what KITTI depth completion calls accumulated lidar ground truth).  The projection and its mask are the
 *       reference's velo2frame + velo2img, sem_pc_accum.py:347-402, on the stored f64 coordinates (owed re-transforms
 *       applied, oldest first) -- the expressions K1 evaluates; the z-buffer itself has no reference counterpart.
 *     cam->P: row-major 3x4, store coordinates -> image, as p_velo_frame.  fx, fy, d = the rows of P as f64 fma chains in
 *       k order; d == 0 -> -1e-6; u = rint(fx / |d|), v = rint(fy / |d|) (IEEE divide).  A point is KEPT iff 0 <= u < width,
 *       0 <= v < height, d > min_depth and d < max_depth (0 and +inf: the reference's mask); a NaN anywhere drops it.
 *     include_dyn == 0: points with dyn == 1 take no part.  only != NULL: neither do points whose class is not in the set.
 *     A kept point competes for every pixel (u + du, v + dv), |du|, |dv| <= radius, that lies inside the image (a square
 *       footprint, clipped, not wrapped; the centre decides whether the point takes part).  A pixel goes to the point with
 *       the smallest (float)d and, among equal ones, the smallest index in the window: the result does not depend on the
 *       order in which points arrive.
 *     Output (dev, all needed; keys is scratch): depth f32 [H][W] ((float)d of the winner, 0 where no point), index i64 [H][W]
 *       (the winner's index relative to the window's first point, -1 where none), rgb u8 [H][W][3] and sem u8 [H][W] (the
 *       winner's colour and class; 0, 0, 0 and 255 where none), stats i64 [3]: points considered (past the dyn and class
 *       filters), points kept by the mask, pixels covered.
 *     Scope: no lens distortion; ONE P per call (no per-frame camera poses); no hidden-point removal beyond the footprint.
 *     Limits: 1 <= width, height, width * height <= 2^24; 0 <= radius <= 3; 0 <= min_depth < max_depth; every entry of P
 *       finite; max_points < 2^32; slot_begin <= slot_end.
 *     The store is never written: owed re-transforms (pending_Ts / pending_slot_ends / n_pending as pca_bev_generate_chain
 *     takes them) are applied to the points that are read and stay owed.  A K1 noted by pca_k1_defer runs on its own first; a
 *     bin range armed by pca_bev_bin_range / pca_bev_view_hint is neither used nor cleared.  A window above max_points is
 *     cut there and raises PCA_STATUS_STORE_OVERFLOW; a window without points gives the empty image.  Every argument is
 *     checked before anything is launched; -1 with pca_last_error set ("render camera: ...").
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    double P[12];              /* row-major 3x4: store coordinates -> image, as p_velo_frame */
    int32_t width, height, radius, include_dyn;
    double min_depth, max_depth;
} pca_camera;
int pca_render_camera(pca_ctx *ctx, const pca_store *store, const int64_t *frame_off /*dev*/,
                      int slot_begin, int slot_end, int64_t max_points, const pca_camera *cam,
                      const pca_class_group *only /* NULL: every class */,
                      const double *pending_Ts, const int *pending_slot_ends, int n_pending,
                      uint64_t *keys /* dev [H][W], scratch */, float *depth /*dev [H][W]*/, int64_t *index /*dev [H][W]*/,
                      uint8_t *rgb /* dev [H][W][3] */, uint8_t *sem /*dev [H][W]*/, int64_t *stats /* dev [3] */,
                      void *stream);

/* ------------------------------------------------------------------------------------------------
 * Camera rays cast through the voxel grid of pca_bev_voxel_labels: which voxels a pinhole camera sees before its ray is
 *       stopped by an occupied voxel -- the "mask_camera" of Occ3D, the ".occluded" of SemanticKITTI-SSC / SSCBench-KITTI-360,
 *       beside the lidar mask of pca_bev_voxel_rays -- and, per ray, the first occupied voxel, its depth and its label.  No
 *       reference counterpart.  One ray per pixel of the (strided) image; occupied is whatever `labels` says (!= 255).
 *     Everything is f64, each operation rounded on its own, nothing fused, the divisions IEEE.
 *     The camera: with P = [M | p4] from store coordinates to the image (as pca_render_camera takes it), the host passes
 *       Minv = inv(M) (row-major 3x3) and C = -Minv p4, the camera centre.  The call never sees P: its results are defined on
 *       Minv and C, however the host got them.
 *     The rays: nu = width / stride, nv = height / stride (integer division).  Ray (i, j), 0 <= i < nu, 0 <= j < nv, goes
 *       through the pixel position u = i stride + (stride - 1) / 2.0, v = j stride + (stride - 1) / 2.0 (pixel centres sit at
 *       integer coordinates, as in K1 and pca_render_camera); its outputs sit at [j][i].
 *       dir_k = (Minv[3k] u + Minv[3k+1] v) + Minv[3k+2];  start S = C;  end E_k = C_k + max_depth dir_k, the point at camera
 *       depth max_depth (no square root).
 *     Grid coordinates s, e of S, E and the voxel of a position: word for word those of pca_bev_voxel_rays, from the same
 *       code.  A ray with a coordinate of s or e that is not finite or is >= 2^30 in magnitude is dropped (stats[2]); with
 *       start voxel c, end voxel g and n_a = |g_a - c_a|, a ray with N = n_0 + n_1 + n_2 > PCA_BEV_RAYS_MAX_STEPS is dropped
 *       (stats[3]).
 *     The walk: set-up, step and tie order (u, v, w) are those of pca_bev_voxel_rays; the ray visits N + 1 voxels c_0 .. c_N
 *       -- unlike a lidar ray, the end voxel counts.  For each visited voxel (i, j, k) inside the grid, in order:
 *       visible[k][px - 1 - j][i] = 1; if labels there is not 255 the ray has HIT: it records the voxel and stops.
 *       t_enter is 0.0 for c_0, else the tMax of the axis that was just stepped, taken before its increment.
 *     Per ray (dev [nv][nu], each may be NULL): hit i32 = the place (k px + (px - 1 - j)) px + i of the hit voxel, -1 without
 *       a hit (a dropped ray included); depth f32 = (float)(t_enter max_depth) of the hit, 0 without; label u8 = labels at
 *       the hit, 255 without.
 *     visible u8 [nz][px][px]: cam->clear != 0: zeroed first; cam->clear == 0: the call marks into what is there (the union
 *       over several cameras).  Every writer writes 1: the result does not depend on any order.
 *     stats i64 [5], zeroed on every call: rays, rays cast (not dropped), dropped not finite, dropped too long, hits.
 *     Scope: ONE pinhole per call; no lens distortion; whether a voxel stops a ray is decided by `labels` alone.
 *     Of prm, origin, R (a rotation about z, checked), dx, dy, view and px are read.
 *     Limits: prm, labels, cam, visible and stats not NULL; width, height, stride >= 1, stride <= min(width, height);
 *       max_depth finite and > 0; every entry of Minv and C finite; 1 <= nz <= 32, z_lo finite, z_step finite and > 0;
 *       1 <= px <= 1024.  No workspace.
 *     The call reads neither the store nor the owed chain and writes only its outputs.  Every argument is checked before
 *     anything is launched or cleared; -1 with pca_last_error set ("bev voxel camera: ..." naming the argument).
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    double Minv[9], C[3];      /* inv(M) row-major and the camera centre -inv(M) p4, for P = [M | p4] */
    int32_t width, height, stride, clear;
    double max_depth;
} pca_ray_camera;
int pca_bev_voxel_camera(pca_ctx *ctx, const pca_bev_params *prm, double z_lo, double z_step, int nz,
                         const uint8_t *labels /*dev [nz][px][px], 255 = empty*/, const pca_ray_camera *cam,
                         uint8_t *visible /*dev [nz][px][px]*/,
                         int32_t *hit /*dev [nv][nu] or NULL*/, float *depth /*dev [nv][nu] or NULL*/, uint8_t *label /*dev [nv][nu] or NULL*/,
                         int64_t *stats /*dev [5]: rays, cast, dropped not finite, dropped too long, hits*/,
                         void *stream);

/* ------------------------------------------------------------------------------------------------
 * Voxel volumes pooled to coarser scales, and packed into the payloads of SemanticKITTI-SSC's files (pca_voxel_pool.hip).  No
 *       reference counterpart.  Both calls read volumes in this library's layout -- u8 [nz][px][px], voxel (i, j, k) at
 *       [k][px - 1 - j][i] -- as pca_bev_voxel_labels, pca_bev_voxel_rays and pca_bev_voxel_camera leave them; neither reads a
 *       store or points.  Everything is integer.
 *     Fine voxel state (both calls): OCCUPIED with label l iff its label byte l is < PCA_BEV_VOXEL_MAX_LABELS -- any other byte
 *       counts as 255, not only 255 itself; else FREE iff its `seen` byte != 0, else UNSEEN.
 *
 * pca_voxel_pool: the scales 1:2, 1:4 and 1:8 in ONE launch, one pass over the fine volume.
 *     A coarse voxel of scale s covers s x s x s fine voxels (k, row, col), aligned at 0; n = s^3.  n_occ, n_free, n_unseen: its
 *       counts of fine voxels; c_l: the number of its occupied fine voxels with label l -- voxels, not points.
 *     It is occupied iff n_occ > 0 && n_occ occ_den >= n occ_num (int64 products).  Occupied: labels = the smallest l with c_l
 *       maximal, state = 2.  Else: labels = 255, state = 1 if n_free > n_unseen, else 0 (a tie is unseen).  visible = 1 iff any
 *       fine `visible` byte != 0, else 0.  With occ_num / occ_den = 1 / 20 this is the published rule of SemanticKITTI-SSC's
 *       coarse labels ("more than 0.95 n of the fine voxels empty -> empty"): at least 1, 4 and 26 occupied fine voxels.
 *     Every scale is decided from the FINE voxels: counts are summed up the hierarchy, decisions never are.
 *     levels: a HOST array of n_levels (1..3) descriptors; each output dev [nz/s][px/s][px/s] or NULL, not all three NULL.  Every
 *       byte of every output that is not NULL is written exactly once.
 *     Limits: 1 <= px <= 1024, 1 <= nz <= 32; scale 2, 4 or 8, none twice; px and nz multiples of every requested scale;
 *       occ_den >= 1, 0 <= occ_num <= occ_den; labels and seen not NULL; a visible output needs the visible input.
 *
 * pca_voxel_pack: the file payloads of ONE level (fine or pooled; px, nz are that level's), one launch.
 *     The place of voxel (i, j, k) in every output is t = (i px + j) nz + k: SemanticKITTI's order with this grid's (i, j, k) as
 *       its (x, y, z), z fastest.
 *     label_out u16 [px px nz], the device's (little-endian) byte order: label_map[l] for an occupied voxel, else empty_value.
 *     Bit streams, ceil(px px nz / 8) bytes each, exactly numpy's packbits of the bits in t order: bit t is bit 7 - t % 8 of byte
 *       t / 8, the padding bits of the last byte are 0.  invalid_bits (needs seen): 1 iff UNSEEN.  occluded_bits (needs visible):
 *       1 iff visible == 0.  bin_bits (needs input_occ): 1 iff input_occ != 0.  Every byte is written exactly once; no atomics.
 *     Each output may be NULL, not all; label_map: HOST u16 [PCA_BEV_VOXEL_MAX_LABELS], needed by label_out.
 *     Limits: 1 <= px <= 1024, 1 <= nz <= 32 (no divisibility condition); labels not NULL.
 *
 * Both: every argument is checked before anything is launched; -1 with pca_last_error set ("voxel pool: ..." / "voxel pack:
 *     ..."), nothing written.  PCA_VOXEL_POOL_G / PCA_VOXEL_PACK_G = 1..2048 cap the workgroups.
 *     Out of scope: votes weighted by point counts; other scales; coarse .occluded / .bin; Occ3D's .npz container; how the fine
 *     volumes are made; banded grids above 1024.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t scale;             /* 2, 4 or 8 */
    uint8_t *labels, *state, *visible;     /* dev [nz/scale][px/scale][px/scale], each may be NULL */
} pca_voxel_pool_level;
int pca_voxel_pool(pca_ctx *ctx, int px, int nz, const uint8_t *labels /*dev, 255 = no point*/, const uint8_t *seen /*dev*/,
                   const uint8_t *visible /*dev or NULL*/, int occ_num, int occ_den,
                   const pca_voxel_pool_level *levels /*host [n_levels]*/, int n_levels, void *stream);
int pca_voxel_pack(pca_ctx *ctx, int px, int nz, const uint8_t *labels /*dev*/, const uint8_t *seen /*dev or NULL*/,
                   const uint8_t *visible /*dev or NULL*/, const uint8_t *input_occ /*dev or NULL*/,
                   const uint16_t *label_map /*host [32]*/, uint16_t empty_value,
                   uint16_t *label_out /*dev or NULL*/, uint8_t *invalid_bits /*dev or NULL*/, uint8_t *occluded_bits /*dev or NULL*/,
                   uint8_t *bin_bits /*dev or NULL*/, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Exact distance transform of a label volume: squared distance, nearest site, its label; fill; TSDF (pca_voxel_distance.hip).
 *       No reference counterpart.  Volumes in this library's layout -- [nz][px][px], voxel (i, j, k) at [k][px - 1 - j][i]; the
 *       call reads no store and no points.  The distance is integer arithmetic; only `tsdf` is floating point.
 *     Sites: a voxel is a site iff its label byte l is < PCA_BEV_VOXEL_MAX_LABELS (any other byte counts as 255, as in
 *       pca_voxel_pool) and bit l of site_labels is set (site_labels NULL: every label).
 *     Distance between the places p = (k, row, col) and s = (k', row', col'):
 *       D(p, s) = w_xy ((row - row')^2 + (col - col')^2) + w_z (k - k')^2, an integer; the two weights express anisotropic voxels
 *       exactly (cells of 0.3125 m and bins of 0.2 m: 625 : 256 measures metres in units of 0.0125 m).
 *     Per voxel, the site that minimises the pair (D, q) lexicographically, q = (k' px + row') px + col' the site's linear place:
 *       a tie in distance goes to the smallest place.  With max_dist2 >= 0, sites with D > max_dist2 do not exist for the voxel.
 *       dist2 = D, nearest = q, nearest_label = the site's label byte; without a site -1, -1 and 255.  A site has dist2 = 0 and
 *       nearest = its own place.
 *     filled: the voxel's own label byte where it is < PCA_BEV_VOXEL_MAX_LABELS (a site or not); else nearest_label where a site
 *       exists with D <= fill_dist2 and the voxel is eligible -- fill_free != 0, or seen == NULL, or its seen byte is 0 (by default
 *       a voxel a beam crossed stays free); else 255.
 *     tsdf, f32, computed in f64 with every operation rounded on its own: m = fmin(sqrt((double)D) * tsdf_unit, tsdf_trunc) /
 *       tsdf_trunc, m = 1 without a site; v = tsdf_flip ? 1.0 - m : m; sign = -1 where seen != NULL, the voxel's label byte is
 *       not < PCA_BEV_VOXEL_MAX_LABELS and its seen byte is 0 (unseen), else +1; out = (float)(sign * v).  SSCNet's convention:
 *       positive in observed space, negative behind surfaces, +-1 at the surface when flipped.
 *     Each output dev [nz][px][px] or NULL, not all five; every element of every output that is not NULL is written exactly once;
 *       no atomics; two calls give identical bytes.  workspace: dev, pca_voxel_distance_workspace_bytes(px, nz) bytes (-1 for a
 *       shape outside the limits), 4-byte aligned.
 *     Limits: 1 <= px <= 1024, 1 <= nz <= 32; w_xy, w_z >= 1 with w_xy 2 (px-1)^2 + w_z (nz-1)^2 <= 2^31 - 2 (every D fits the
 *       int32 output); labels not NULL; tsdf needs tsdf_unit and tsdf_trunc finite and > 0; filled needs fill_dist2 >= 0 (< 0: no
 *       fill).  max_dist2 < 0: unbounded.
 *     Every argument is checked before anything is launched; -1 with pca_last_error set ("voxel distance: ..."), nothing written.
 *       Two launches whatever the volume holds.  PCA_VOXEL_DIST_G = 1..2048 caps the workgroups of both.
 *     Out of scope: distances in float metres for irrational cell ratios; grids above 1024; a .tsdf file; distance to free-space
 *     boundaries; how the fine volumes are made.
 * ------------------------------------------------------------------------------------------------ */
int64_t pca_voxel_distance_workspace_bytes(int px, int nz);
int pca_voxel_distance(pca_ctx *ctx, int px, int nz, const uint8_t *labels /*dev*/, const uint8_t *seen /*dev or NULL*/,
                       const pca_class_group *site_labels /*host or NULL = every label*/, int w_xy, int w_z,
                       int64_t max_dist2 /* <0: unbounded */, int64_t fill_dist2 /* <0: no fill */, int fill_free,
                       double tsdf_unit, double tsdf_trunc, int tsdf_flip, void *workspace /*dev*/, int64_t workspace_bytes,
                       int32_t *dist2, int32_t *nearest, uint8_t *nearest_label, uint8_t *filled, float *tsdf /*each dev or NULL, not all*/,
                       void *stream);

/* ------------------------------------------------------------------------------------------------
 * The instances of one sample matched to those of the sample before it: stable ids over a sequence (pca_voxel_match.hip).
 *       No reference counterpart.  Two instance volumes in this library's layout -- i32 [nz][px][px], -1 = no instance, what
 *       pca_bev_voxel_instances writes as `inst`, though any i32 volume is legal -- and a map between their index spaces; the
 *       call reads no store and no points.  Integer counts and maxima only, apart from the map itself.
 *     Ids: a voxel of `cur` (`prev`) takes part iff 0 <= id < n_cur (n_prev); an id >= its row count or < -1 is skipped and
 *       counted in stats[8] (stats[9]); it is not an error.
 *     The map: M, HOST f64 [12], row-major 3 x 4, from the continuous index of a cur voxel centre to a continuous index in
 *       prev (pca_amd.host_logic.voxel_index_map makes it from two grids and the rigid map between them).  Everything is f64,
 *       every operation rounded on its own, no fma.  For a voxel (k, row, col) of cur with id b: u = col + 0.5, v = row + 0.5,
 *       w = k + 0.5; q_i = ((M[i][0] u + M[i][1] v) + M[i][2] w) + M[i][3], i = 0, 1, 2: col', row', k'.  The image is IN VIEW
 *       iff 0 <= q_0 < px && 0 <= q_1 < px && 0 <= q_2 < nz, tested on the f64 values before any conversion (a NaN is out of
 *       view).  Then a = prev[floor q_2][floor q_1][floor q_0]; if 0 <= a < n_prev the pair (a, b) gains one.
 *     C(a, b): the pair's count.  vox_cur[b]: the voxels of b in cur; in_view[b]: those whose image is in view; vox_prev[a]:
 *       the voxels of a in prev.  best_prev(b): the a with the largest C(a, b) > 0, the smallest a among equal ones;
 *       best_cur(a): the b with the largest C(a, b) > 0, the smallest b among equal ones.
 *     b MATCHES a iff a = best_prev(b) && b = best_cur(a) && C >= min_overlap &&
 *       (double)C >= min_iou * (double)(vox_prev[a] + vox_cur[b] - C) (one rounded product).
 *     Tracks, t0 = *track_counter on entry: a matched b takes prev_track[a] (prev_track NULL: a itself); an unmatched b with
 *       vox_cur[b] > 0 takes t0 + its rank among such b in ascending b; a row with vox_cur[b] = 0 takes -1 and uses up no
 *       number; *track_counter leaves the call as t0 + the number of new tracks.  track_counter is read AND written on the
 *       device, on the stream: calls chain without a host read.
 *     Outputs, all dev, each may be NULL but not all, each fully written:
 *       cur_track i32 [n_cur]; match i32 [n_cur]: the matched a or -1;
 *       cur_info u32 [n_cur][4]: vox_cur, in_view, C at best_prev, best_prev + 1 (0: none);
 *       prev_info u32 [n_prev][4]: vox_prev, C at best_cur, best_cur + 1, the matched b + 1;
 *       track_vol i32 [nz][px][px]: cur_track of the voxel's id, -1 without a row;
 *       track_ids i32 [n_ids]: cur_track of ids[p] (ids: dev i32 [n_ids], e.g. pca_bev_voxel_instances' per-point ids of cur),
 *         -1 where the id is outside 0 .. n_cur - 1;
 *       pairs u32 [cap_pairs][3]: a, b, C in NO defined order, unused rows 0xffffffff in all three words;
 *       stats i64 [10]: cur voxels with a row, of which in view, sum of C, distinct pairs, dropped increments, matched, new
 *         tracks, prev rows with vox_prev > 0 left unmatched (lost), cur voxels skipped, prev voxels skipped.
 *     The pair table: open addressing over cap_pairs slots of the workspace with a BOUNDED probe; after cap_pairs probes an
 *       increment is given up and counted in stats[4]; nothing spins, nothing waits.  With stats[4] > 0 only stats[0..1],
 *       that stats[4] is > 0 (which increments were lost depends on the order of arrival), stats[8..9], vox_cur, in_view and
 *       vox_prev are defined; the Python layers raise.
 *     Every defined output but the order of `pairs` is a function of the two volumes and M alone: bests are 64-bit atomic
 *       maxima of (C << 32 | ~id), counts are integer sums.
 *     workspace: dev, pca_voxel_instance_match_workspace_bytes(n_prev, n_cur, cap_pairs) bytes (-1 outside the limits), 8-byte
 *       aligned.
 *     Limits: 1 <= px <= 1024, 1 <= nz <= 32; 1 <= n_prev, n_cur <= 65536; every entry of M finite; min_overlap >= 1; min_iou
 *       finite, 0 .. 1; cap_pairs a power of two, 16 .. 2^22; prev, cur, M, track_counter not NULL; track_ids needs ids.
 *     Every argument is checked before anything is launched; -1 with pca_last_error set ("voxel instance match: ..."), nothing
 *       written.  Five launches whatever the volumes hold (four when neither track_vol nor track_ids is asked for); no wait on
 *       the device or between workgroups.  PCA_VOXEL_MATCH_G = 1..2048 caps the workgroups; PCA_VOXEL_MATCH_FOLD=0 turns the
 *       folding of equal keys within a wave off (same results).  The kernels carry no id of pca_profile_read.
 *     min_overlap = 1 and min_iou = 0 are the shipped defaults of the Python layers: this project's choice, checked on
 *       synthetic scenes only.
 *     Out of scope: motion models or prediction, re-identifying a track after a sample in which it was unmatched, merging or
 *     splitting instances, Hungarian or other globally optimal assignment, velocities, different px or nz between the samples.
 * ------------------------------------------------------------------------------------------------ */
int64_t pca_voxel_instance_match_workspace_bytes(int n_prev, int n_cur, int cap_pairs);
int pca_voxel_instance_match(pca_ctx *ctx, int px, int nz, const int32_t *prev /*dev*/, int n_prev, const int32_t *cur /*dev*/, int n_cur,
                             const double *M /*host [12]*/, int min_overlap, double min_iou, int cap_pairs,
                             const int32_t *prev_track /*dev [n_prev] or NULL*/, int32_t *track_counter /*dev [1], read and written*/,
                             const int32_t *ids /*dev [n_ids] or NULL*/, int64_t n_ids, void *workspace /*dev*/, int64_t workspace_bytes,
                             int32_t *cur_track, int32_t *match, uint32_t *cur_info, uint32_t *prev_info, int32_t *track_vol,
                             int32_t *track_ids, uint32_t *pairs, int64_t *stats /*each dev or NULL, not all*/, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Input normalisation of the semseg CNN on the device.  Replaces utils/onnx_utils.py:26-29, :35-36
 *     (torchvision ToTensor + Normalize on the host): out[c][y][x] = (rgb[y][x][c] / 255 - mean[c]) / std[c] in IEEE f32.
 *     rgb: dev [H,W,3] u8; out: dev [3,H,W] f32.  The CNN itself is an external ONNX file (utils/onnx_utils.py binds this
 *     buffer and the class-map output to an onnxruntime session, so neither visits the host).
 * ------------------------------------------------------------------------------------------------ */
int pca_image_to_nchw_f32(pca_ctx *ctx, const uint8_t *rgb /*dev*/, int H, int W, const float mean[3], const float std[3],
                          float *out /*dev*/, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Polynomial warp of finished fp16 planes (--bev_do_warp augmentation).  Replaces
 *       bev_generator/bev_generator.py:482-525 (warp_dense_probmaps: a Python loop over px^2 cells).
 *     out[n][jw][iw] = in[n][clamp(rint(b_1 jw + b_2 jw^2))][clamp(rint(a_1 iw + a_2 iw^2))], the index expressions
 *     evaluated exactly as numpy evaluates them; (a_1, a_2) / (b_1, b_2) come from cal_warp_params (:563-569).
 *     planes_f16, out_f16: dev [n_planes, px, px], distinct buffers.
 * ------------------------------------------------------------------------------------------------ */
int pca_bev_warp(pca_ctx *ctx, const uint16_t *planes_f16 /*dev*/, uint16_t *out_f16 /*dev*/, int n_planes, int px,
                 double a_1, double a_2, double b_1, double b_2, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Host helper (no device work): the ego trajectory of one BEV sample -- rotate, translate, clip to the view box
 * with bisected border crossings, grid coordinates.  Replaces bev_generator/bev_generator.py:207-371, :737-747 for
 * the ego polyline (plain IEEE arithmetic, bit-identical to the numpy form in pca_amd/host_logic.py; the rotation's sums
 * begin from +0.0 as numpy's do, which decides the sign of a zero z).
 * full: host [F,3] f64; R: 3x3 row-major; rows: host [2(F-1),3] out; start: host [F] out (first row of every
 * edge; start[F-1] = number of rows).  Returns the number of rows.
 * ------------------------------------------------------------------------------------------------ */
int pca_host_ego_to_grid(const double *full, int F, const double R[9], double dx, double dy, double view, int px,
                         double *rows, int32_t *start);

/* ------------------------------------------------------------------------------------------------
 * KL  the ground-truth lane centrelines of a whole map, clipped to the BEV of S samples in one launch set.
 *     Replaces bev_generator/bev_generator.py:101-109 (preprocess_pc_and_trajs on a dummy cloud with every lane, then the
 *     non-empty filter) with geometric_transform(is_traj=True) :207-237, crop_trajectory / cal_intersec_pnt :257-371 and
 *     pos2grid :737-747 underneath, as nuscenes_oracle_sem_pc_accum.py:173-176, :552-554 feed it (lane - bev_frame_coords),
 *     and the once-per-scene homo_transform per lane of nuscenes_oracle_sem_pc_accum.py:71, :171.
 *     The lane set: xyz dev [P,3] f64, the vertices of the L lanes one after the other; start dev [L+1] i32, lane i owns
 *     vertices start[i] .. start[i+1]-1; vertex_lane dev [P] i32, the lane of every vertex (an edge joins two consecutive
 *     vertices of the same lane; the present kernels read the lane boundaries from vertex_lane alone).
 * pca_lanes_transform  xyz <- (T [p; 1])[:3] in place (T: host, 4x4 row-major): the f64 fma chain in k order of K1n / K2,
 *     bit-equal to datasets.nuscenes_utils.homo_transform lane by lane.
 * pca_lanes_to_grid    per sample k and edge a -> b, with the roundings of pca_host_ego_to_grid on (lane - views[k].origin):
 *     an inside `a` gives a row, an edge with exactly one end inside additionally the bisected crossing carrying a's z; x, y
 *     are floor(v / view * px + 0.5 px).  rows: dev [S][cap_rows][3] f64 in edge order (= map order); row_lane: dev
 *     [S][cap_rows] the row's lane; n_rows: dev [S] the TRUE count -- rows beyond cap_rows are not written: run that sample
 *     again with cap_rows >= n_rows.  ws: dev, pca_lanes_workspace_bytes(P, S, cap_rows) bytes.  Three launches and a fetch of
 *     the views, no synchronisation; P < 2, L == 0: n_rows is zeroed, nothing is launched; S == 0: nothing is done.  A
 *     crossing not found within 1100 halvings raises PCA_STATUS_LANES_BISECT_CAP (no finite input gets there).
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    double origin[3];          /* bev_frame_coords: subtracted from every vertex first */
    double R[9];               /* rotation, row-major */
    double dx, dy, view;       /* shift [m], aug_view_size [m] */
    int32_t px, reserved;      /* pixel_size */
} pca_lane_view;
int64_t pca_lanes_workspace_bytes(int64_t n_vertices, int n_samples, int64_t cap_rows);
int pca_lanes_transform(pca_ctx *ctx, double *xyz /*dev*/, int64_t P, const double T[16], void *stream);
int pca_lanes_to_grid(pca_ctx *ctx, const double *xyz /*dev*/, const int32_t *vertex_lane /*dev*/, const int32_t *start /*dev*/,
                      int64_t P, int32_t L, const pca_lane_view *views /*host [S]*/, int S, int64_t cap_rows,
                      double *rows /*dev [S][cap][3]*/, int32_t *row_lane /*dev [S][cap]*/, int64_t *n_rows /*dev [S]*/, void *ws,
                      void *stream);

/* ------------------------------------------------------------------------------------------------
 * One library call per driver call (KITTI-360 flow).  The reference's driver calls integrate(observations) per frame and
 * generate_bev(present_idx, bev_num, gen_future) when its trigger fires (run_kitti360_bev_gen.py:186-273); each of the two
 * below does everything the library contributes to one such call.
 *
 * pca_kitti_integrate  replaces kitti360_sem_pc_accum.py:41-88: K1 on the observation (see pca_kitti_project_sample_filter)
 *     + the pose bookkeeping of the frame (pca_host_track_step; track may be NULL: the caller keeps its own).  Inputs named
 *     in host_mask are HOST arrays (what the reference's loader yields: kitti360_obs_dataloader.py:87-106); they are copied
 *     into a pinned block of the context on the staging pool and leave in ONE asynchronous H2D copy; the others are device
 *     pointers.  frame_off[slot] must hold the append position; *evicted / *path_length as pca_host_track_step.
 *     K1's checks of the frame (pca_kitti_project_sample_filter_ex: sample mode, pts with n > 0, H and W, rgb + sem or
 *     sem_gt) run FIRST, with pca_k1_defer on as well: a refused frame is neither staged nor noted, the track is not
 *     stepped and *evicted / *path_length are left alone.
 * pca_kitti_generate_bev  replaces kitti360_sem_pc_accum.py:166-243 + bev_generator.py:63-125 for one un-augmented sample:
 *     ego polylines (pca_host_ego_to_grid on poses - prm->origin; rows / start / *n_rows as there, F = poses of the track
 *     = slot_end - slot_begin), raster (pca_bev_generate_chain, same arguments), and -- host_planes != NULL: page-locked,
 *     21 px px 2 bytes -- the planes' copy to the host (pca_host_d2h_async).  Returns that copy's ticket (0 without), -1 on error.
 * ------------------------------------------------------------------------------------------------ */
typedef struct pca_host_track pca_host_track;
typedef struct {
    const void *pts;       /* [n,4] f32 x,y,z,intensity                                        */
    const void *rgb;       /* [H,W,3] u8, or NULL with sem_gt                                  */
    const void *sem;       /* [H,W] u8 class map, or NULL with sem_gt                          */
    const void *sem_gt;    /* [n] u8 per-point class, or NULL                                  */
    int32_t n;
    uint32_t host_mask;    /* bit 0 pts, 1 rgb, 2 sem, 3 sem_gt: that pointer is a HOST array  */
} pca_kitti_obs;
int pca_kitti_integrate(pca_ctx *ctx, const pca_kitti_obs *obs, const double P[12], int H, int W,
                        const uint64_t filter_mask[4], const pca_store *store, int64_t *frame_off /*dev*/, int slot,
                        int sample_mode, pca_host_track *track, const double *T_new_prev, double horizon, int64_t *evicted,
                        double *path_length, void *stream);
/* Frames that cannot reach the view, skipped by a raster.  The window of a sample spans the accumulation horizon, the view a
 * part of it: the frames far ahead of the sample's pose and the oldest ones put no point into any plane, yet the raster's
 * first kernel loads and transforms them.  The CALLER knows where every frame is:
 * pca_host_view_hull (host only, no GPU): frame f of F (oldest first) was created when the product of all transforms applied to
 *     the store was then[f] (3x4 row-major; the caller multiplies every T onto its running product `now`: the reference's
 *     update_sem_pcs, sem_pc_accum.py:168-183), so its points are, now, at  now * inverse(then[f]) * (where K1 put them);
 *     K1 only keeps points in front of the camera whose pixel lies in the image, i.e. inside the cone `cone` (apex, then the four
 *     rays through the image corners, in the sensor's frame: pca_host_camera_cone; NULL: no camera test, e.g. per-point
 *     labels) and inside box[f] (six floats lo/hi per coordinate, what K1 left in pca_store.frame_box; lo > hi = unknown).  Returns in
 *     *first / *last the first and the last frame for which neither the cone nor the box proves that it misses the view square of prm (1 cm of
 *     margin; -1 / -1: none); every frame outside [first, last] is certain to fail the raster's crop with all its points.
 * pca_bev_bin_range: the NEXT pca_bev_generate_chain / pca_kitti_generate_bev of the context bins the slots [slot_first,
 *     slot_last_plus1) only (clamped to its window; ignored, and forgotten, if that call writes owed transforms back or is a
 *     pca_bev_generate_many).  Results do not change when every frame outside has no point in the view.  A range is good for
 *     ONE call and never outlives it: the raster takes it and forgets it whether it succeeds or is refused; a
 *     pca_kitti_generate_bev[_v] that returns -1 before its raster leaves nothing armed; a later pca_bev_bin_range or
 *     pca_bev_view_hint REPLACES it (slot_last_plus1 < slot_first: nothing is armed). */
void pca_host_camera_cone(const double P[12], int H, int W, double cone[15]);
int pca_host_view_hull(int F, const double *then /*[F][12]*/, const float *box /*[F][6]*/, const double *cone /*[15] or NULL*/,
                       const double now[12], const pca_bev_params *prm, int *first, int *last);
int pca_bev_bin_range(pca_ctx *ctx, int slot_first, int slot_last_plus1);
/* the two in one call (frame 0 of the F frames sits in slot0): 1 = a narrower range was set, 0 = every frame may reach the view,
 * -1 = bad arguments.  The hint replaces whatever was armed before it: after 0 or -1 NO range is armed. */
int pca_bev_view_hint(pca_ctx *ctx, int slot0, int F, const double *then, const float *box, const double *cone, const double now[12],
                      const pca_bev_params *prm);
void pca_f32_box_decode(const uint32_t *rows /*[n][6]*/, int n, float *box /*[n][6]: lo x, hi x, lo y, ...; lo > hi = empty*/);

/* Diagnostics (read only; nothing here changes what a call computes).
 * pca_debug_bev_level1: level 1's grid as the context's last pca_bev_generate_chain (pca_kitti_generate_bev included) launched
 *     it: out = {G workgroups, Gk of them tiles of a riding K1, bin_first, bin_end: the slots level 1 read from the store --
 *     the window, or what pca_bev_bin_range / pca_bev_view_hint left of it}.  G == the device's compute units with a bin range
 *     set: a one-round launch.  0 / -1. */
int pca_debug_bev_level1(const pca_ctx *ctx, int out[4]);
/* pca_debug_bev_lds: level 1's LDS as the PROCESS's last pca_bev_generate_chain launched it (process-wide: read it before another
 *     context of the process rasters): out = {points per thread parked in LDS behind the register points (0, or 4 where the
 *     CU's LDS has room; PCA_BEV_LDS_P=0: always 0), bytes of dynamic LDS: histogram + cursors + the parked block}.  0 / -1. */
int pca_debug_bev_lds(int out[2]);
/* pca_debug_icp_layout: where a pca_icp_register(n_src, n_tgt) leaves its intermediate results in the caller's workspace
 *     (host only; nothing is launched).  out[0..11]: byte offsets, from the workspace's base rounded up to 256, of start[0],
 *     spts[0] (coarse grid), start[1], spts[1] (fine grid), normal, nn_prev, nn_cell, nn_slack, partial, zr_part, state, and the
 *     total; out[12..15]: the doubles of the state block at which the four slab-range words and the sums of the last pass
 *     lie, the number of those sums, and the cells per grid (start[] has one word more).  0 / -1 (n < 1, out == NULL). */
int pca_debug_icp_layout(int32_t n_src, int32_t n_tgt, int64_t out[16]);

/* K1 of pca_kitti_integrate left for the raster that follows it.  The reference's driver integrates a frame and, when its
 * trigger fires, rasterises the window that ends with that frame (run_kitti360_bev_gen.py:186-273): with on = 1, a
 * pca_kitti_integrate whose inputs are the plain kind (nearest sampling; rgb + class map, or per-point labels) does the pose bookkeeping and the
 * staging as before but only NOTES its K1; the next pca_bev_generate_chain / pca_kitti_generate_bev of the context whose
 * window ends with that slot (same store, frame_off and stream, 5 planes x int32 layout) runs it as the first workgroups
 * of its own first kernel -- the frame's kept points go into the store AND, straight from registers, into the raster's
 * tile lists, so they are not read back.  Every other entry point that reads or writes a store runs a noted K1 first, on
 * its own (the order of effects on `stream` is the order of the calls, as without deferral); so does pca_status.  Until
 * then -- the next library call on the context -- the DEVICE buffers of the observation must stay UNMODIFIED, not only
 * allocated: the noted K1 reads them when it runs (host arrays are held in the context's staging block).
 * pca_k1_defer(ctx, 0) turns it off and runs what is noted; pca_k1_flush runs what is noted.  0 / -1. */
int pca_k1_defer(pca_ctx *ctx, int on);
int pca_k1_flush(pca_ctx *ctx);
int pca_kitti_generate_bev(pca_ctx *ctx, const pca_store *store, const int64_t *frame_off /*dev*/, int slot_begin,
                           int slot_split, int slot_end, int64_t max_points, const pca_bev_params *prm,
                           const double *pending_Ts, const int *pending_slot_ends, int n_pending, int write_back,
                           void *workspace /*dev*/, int64_t workspace_bytes, uint16_t *planes_f16 /*dev*/,
                           void *host_planes /*pinned or NULL*/, const pca_host_track *track, double *traj_rows,
                           int32_t *traj_start, int32_t *n_rows, void *stream);

/* The same two calls with their arguments in a block the caller keeps between calls: a binding in an interpreted language
 * (ctypes: ~0.2 us per converted argument, 45 arguments per step) rewrites the few fields that change -- slot numbers, the
 * pose, the output pointers -- and passes two pointers.  Members as the parameters of the same name; `evicted`, `path_length`,
 * `n_rows` are outputs.  pca_kitti_generate_bev_v also takes the view hint (hint_F > 0: the arguments of pca_bev_view_hint;
 * it is skipped, like the hint itself, when the call writes owed transforms back).  Returns what the plain form returns; a
 * call that returns -1 -- a bad hint, a refused argument, a refused raster -- leaves no bin range armed for a later raster. */
typedef struct {
    const pca_kitti_obs *obs; const double *P; int32_t H, W; const uint64_t *filter_mask; const pca_store *store;
    int64_t *frame_off; int32_t slot, sample_mode; pca_host_track *track; const double *T_new_prev; double horizon;
    int64_t evicted; double path_length; void *stream;
} pca_kitti_integrate_args;
int pca_kitti_integrate_v(pca_ctx *ctx, pca_kitti_integrate_args *a);
typedef struct {
    const pca_store *store; const int64_t *frame_off; int32_t slot_begin, slot_split, slot_end, pad0; int64_t max_points;
    const pca_bev_params *prm; const double *pending_Ts; const int *pending_slot_ends; int32_t n_pending, write_back;
    void *workspace; int64_t workspace_bytes; uint16_t *planes_f16; void *host_planes; const pca_host_track *track;
    double *traj_rows; int32_t *traj_start; int32_t n_rows, pad1; void *stream;
    int32_t hint_slot0, hint_F; const double *hint_then; const float *hint_box; const double *hint_cone; const double *hint_now;
    int32_t hinted, pad2;          /* out: 1 if the hint left frames out */
} pca_kitti_generate_bev_args;
int pca_kitti_generate_bev_v(pca_ctx *ctx, pca_kitti_generate_bev_args *a);

/* ------------------------------------------------------------------------------------------------
 * Host arrays -> device for callers that hold their observations in pageable host memory -- what the reference's drivers
 * pass to integrate() (run_kitti360_bev_gen.py:173-190: numpy arrays straight from the loader).  src[k] (pageable, bytes[k]
 * long) is copied into pinned[k] (page-locked, caller-owned, at least bytes[k]) on a small pool of host threads, then
 * pinned[k] -> dev[k] is enqueued on `stream` (asynchronous).  The pinned blocks may be reused once the stream has passed
 * the copies (record an event after the call).  PCA_STAGING_THREADS (default 3; 0 = the calling thread alone) and
 * PCA_STAGING_SPIN_US (default 2000: how long the pool's threads poll after a job before they sleep) tune the pool.
 * Returns 0, -1 for bad arguments, -2 if a copy could not be enqueued.
 * ------------------------------------------------------------------------------------------------ */
int pca_host_stage_h2d(int n, const void *const *src, void *const *pinned, void *const *dev, const int64_t *bytes,
                       void *stream);

/* ------------------------------------------------------------------------------------------------
 * A device result on its way to the host (the BEV planes of a sample: sem_bev.py hands them back as host float16
 * arrays, bev_generator/sem_bev.py:164-205 of the reference) without the caller's stream waiting for the copy: it runs on
 * a side stream of the context behind everything enqueued on `stream` so far.  `pinned`: page-locked, caller-owned, to be
 * left alone until pca_host_d2h_wait(ticket) has returned.  Returns the ticket (0..63) or -1.
 * ------------------------------------------------------------------------------------------------ */
int pca_host_d2h_async(pca_ctx *ctx, const void *dev, void *pinned, int64_t bytes, void *stream);
int pca_host_d2h_wait(pca_ctx *ctx, int ticket);

/* ------------------------------------------------------------------------------------------------
 * KZ: the gzip container of a sample, compressed on the device.  Replaces the gzip.open(...).write(pickle.dumps(obj)) of
 * sem_pc_accum.py:280-294 for the bytes that live on the device (the fp16 planes, 2.75 MB of a sample's pickle); what
 * comes out is read by the unchanged read_compressed_pickle (:296-302) and inflates to the very bytes the host would have
 * pickled.  Opt-in (pca_amd/writer.py, codec='device'); no reference counterpart for the encoder itself.
 *
 * pca_deflate_chunks   src: device bytes; chunk_table: device, n_chunks entries (offset into src, length 0 ..
 *     PCA_DEFLATE_CHUNK_MAX; any alignment, odd lengths too).  Every chunk becomes one self-contained, byte-aligned piece of
 *     a raw DEFLATE stream: a non-final fixed-Huffman block (BTYPE 01) of literals and of matches of length 3 .. 128 at distance 1
 *     or 2 -- byte runs and half-word runs, split every 128 bytes of the chunk -- that never reach before the chunk's first byte, then an empty non-final stored block
 *     (the sync-flush marker 00 00 ff ff).  Pieces therefore concatenate bytewise, with each other and with stored blocks.
 *     A chunk of n bytes gives at most PCA_DEFLATE_BOUND(n) bytes (no stored-block fallback: random bytes grow by 1/8).
 *     out_sizes[c]: bytes of piece c; out_crcs[c]: CRC-32 (the gzip polynomial, reflected) of the chunk's own bytes;
 *     out: the pieces back to back in table order, piece c at the sum of the sizes before it (room for the sum of the
 *     bounds); workspace: pca_deflate_workspace_bytes(n_chunks), device.  All outputs are device memory.
 *     Stream and lifetime rules are those of pca_host_d2h_async: the kernels run on the context's side stream behind
 *     everything enqueued on `stream` so far, and the return value is a ticket for pca_host_d2h_wait (or -1).  A
 *     pca_host_d2h_async issued after it copies the results behind the kernels.  src, the table, the outputs and the
 *     workspace are to be left alone until the ticket (or a later one) has been waited for.
 * pca_deflate_chunks_dyn   the same call -- signature, workspace, ticket, stream and lifetime rules, outputs, bound -- with
 *     an entropy coder chosen per chunk: the piece is the smaller of the fixed-Huffman piece pca_deflate_chunks makes and a
 *     dynamic-Huffman piece (BTYPE 10) of the very same tokens, decided by exact bit count, a tie going to fixed; so no
 *     piece is larger than pca_deflate_chunks makes it.  The block type of a piece is bits 1-2 of its first byte.  The
 *     literal/length code is a Huffman code of the chunk's own token histogram limited to 15 bits (optimal whenever the
 *     unlimited tree is no deeper), sent up to the highest used symbol; the distance code always is two one-bit codes
 *     (distances 1 and 2); the code lengths go through one fixed, complete code-length code with its run symbols.
 * pca_host_crc32_combine   CRC-32 of A || B from crc(A), crc(B) and the length of B (GF(2) arithmetic, no data pass;
 *     zlib's crc32_combine, which Python's zlib module does not expose).  len_b < 0: returns 0.
 * pca_host_gzip_assemble   one gzip member from n_pieces pieces in order: the 10-byte header, the pieces, a final empty
 *     fixed block, CRC-32 and ISIZE of the whole uncompressed stream.  raw_bytes[k] < 0: piece[k] is piece_bytes[k] plain
 *     bytes (a fragment of the pickle that lives on the host), written as non-final stored blocks of at most 65 535 bytes
 *     and summed here; raw_bytes[k] >= 0: piece[k] is a byte-aligned piece of a DEFLATE stream without a final block (one
 *     or more pieces of pca_deflate_chunks) that inflates to raw_bytes[k] bytes whose CRC-32 is crc[k].  Zero-length
 *     pieces are legal.  Returns the member's length, -1 for bad arguments, -2 if out_cap is too small (20 bytes, every
 *     piece, and 5 bytes per stored block).  Host only.
 * ------------------------------------------------------------------------------------------------ */
#define PCA_DEFLATE_CHUNK_MAX 32768
#define PCA_DEFLATE_MAX_CHUNKS (1 << 20)
#define PCA_DEFLATE_BOUND(n) ((9 * (int64_t)(n) + 7) / 8 + 16)
typedef struct { int64_t offset; int32_t length; int32_t reserved; } pca_deflate_chunk;
int64_t pca_deflate_workspace_bytes(int64_t n_chunks);
int pca_deflate_chunks(pca_ctx *ctx, const void *src /*dev*/, const pca_deflate_chunk *chunk_table /*dev*/, int64_t n_chunks,
                       void *out /*dev*/, uint32_t *out_sizes /*dev*/, uint32_t *out_crcs /*dev*/, void *workspace /*dev*/,
                       void *stream);
int pca_deflate_chunks_dyn(pca_ctx *ctx, const void *src /*dev*/, const pca_deflate_chunk *chunk_table /*dev*/, int64_t n_chunks,
                           void *out /*dev*/, uint32_t *out_sizes /*dev*/, uint32_t *out_crcs /*dev*/, void *workspace /*dev*/,
                           void *stream);
uint32_t pca_host_crc32_combine(uint32_t crc_a, uint32_t crc_b, int64_t len_b);
int64_t pca_host_gzip_assemble(int32_t n_pieces, const void *const *piece, const int64_t *piece_bytes, const int64_t *raw_bytes,
                               const uint32_t *crc, void *out, int64_t out_cap);

/* ------------------------------------------------------------------------------------------------
 * KP: the preview sheet of a BEV sample as a PNG made on the device.  Replaces, opt-in (PCA_VIZ=device, pca_amd/preview.py),
 * the matplotlib figure the drivers save beside every sample (run_kitti360_bev_gen.py:267-270 of the reference calls
 * viz_bev); the layout of the picture is this library's own.
 *
 * The sheet of one sample [21,px,px] f16 (set-major, 7 planes per set) is an RGB8 image 3 px high and 5 px wide: row block s
 * = the set, column block c = the panel road, intensity, rgb, dynamic, elevation (planes 7 s + {0, 1, 2..4, 5, 6}); pixel
 * (r, q) of a panel shows plane element [r][q].  A scalar panel maps v (f16 -> f32) to lut[clamp(floor((v - lo) * scale), 0,
 * 255)] in f32 (NaN -> 0, +inf -> 255, -inf -> 0); the rgb panel to floor(min(max(v, 0), 1) * 255 + 0.5) per channel (NaN ->
 * 0).  Polylines of a (sample, set) are drawn in (255, 0, 0), one pixel wide, over all five panels of that row block: grid
 * point (x, y) is panel pixel column x, row px - 1 - y; a segment (x0, y0) -> (x1, y1) with n = max(|dx|, |dy|) covers, for
 * s = 0 .. n, (x0 + floordiv(2 s dx + n, 2 n), y0 + floordiv(2 s dy + n, 2 n)) (the one point when n = 0); points outside
 * the grid are skipped; a polyline of one vertex is one point.  Coordinates beyond +-2^29 are taken as +-2^29.
 *
 * pca_preview_stream_bytes   (1 + 15 px) * 3 px: the PNG scanline stream of one sheet (-1: px outside 1 .. 4096).
 * pca_preview_sheets   planes: device [k,21,px,px] f16; verts: device [n_verts][2] int32 (x, y); polylines: device,
 *     n_polylines records (an entry that names no sample, set or vertices of the call is skipped); lut: device [256][3] u8;
 *     ranges: HOST [4][2] f32, (lo, scale) of road, intensity, dynamic, elevation, scale = 256 / (hi - lo); filter: the PNG
 *     filter of every scanline, 0 None, 1 Sub (3 bytes per pixel), 2 Up.  Writes to out_stream (device, k *
 *     pca_preview_stream_bytes(px), any alignment) the scanlines of every sheet, each one filter-type byte and 15 px
 *     filtered bytes, overlay included; nothing else is written.  workspace: pca_preview_workspace_bytes(k, px), device.
 * pca_adler32_chunks   out[c] (device) = Adler-32, from the initial value 1, of chunk c of chunk_table (device; lengths as
 *     for pca_deflate_chunks) alone: zlib.adler32(chunk).  A zero-length chunk gives 1.
 *     Both calls follow pca_deflate_chunks' stream and lifetime rules: the context's side stream, behind everything enqueued
 *     on `stream`, the return value a ticket for pca_host_d2h_wait (or -1).
 * pca_host_adler32_combine   Adler-32 of A || B from adler(A), adler(B) and the length of B (zlib's adler32_combine).
 *     len_b < 0: returns 0.
 * pca_host_png_assemble   one PNG: signature, IHDR (8 bits, colour type 2, no interlace), ONE IDAT holding the zlib header
 *     78 01, the pieces in order (byte-aligned pieces of a DEFLATE stream without a final block, as pca_deflate_chunks makes
 *     them of the chunks of a scanline stream), a final empty fixed block and `adler` (of the whole scanline stream), IEND;
 *     chunk CRCs are computed here.  Returns the file's length, -1 for bad arguments (an IDAT beyond 2^31 - 1 bytes
 *     included), -2 if out_cap is too small (65 bytes and every piece).  Host only.
 * ------------------------------------------------------------------------------------------------ */
#define PCA_PREVIEW_MAX_PX 4096
typedef struct { int32_t sample, set, first, count; } pca_preview_polyline;
int64_t pca_preview_stream_bytes(int32_t px);
int64_t pca_preview_workspace_bytes(int32_t k, int32_t px);
int pca_preview_sheets(pca_ctx *ctx, const void *planes /*dev*/, int32_t k, int32_t px, const int32_t *verts /*dev*/, int64_t n_verts,
                       const pca_preview_polyline *polylines /*dev*/, int32_t n_polylines, const uint8_t *lut /*dev*/,
                       const float *ranges /*host*/, int32_t filter, void *out_stream /*dev*/, void *workspace /*dev*/, void *stream);
int pca_adler32_chunks(pca_ctx *ctx, const void *src /*dev*/, const pca_deflate_chunk *chunk_table /*dev*/, int64_t n_chunks,
                       uint32_t *out /*dev*/, void *stream);
uint32_t pca_host_adler32_combine(uint32_t adler_a, uint32_t adler_b, int64_t len_b);
int64_t pca_host_png_assemble(int32_t width, int32_t height, int32_t n_pieces, const void *const *piece, const int64_t *piece_bytes,
                              uint32_t adler, void *out, int64_t out_cap);

/* ------------------------------------------------------------------------------------------------
 * Host helper (no device work): the accumulator's pose track -- the per-frame bookkeeping integrate() does on Python
 * lists in the reference.  Replaces sem_pc_accum.py:156-165 (update_poses), :185-209 (remove_observations), :211-228
 * (comp_incr_path_dist), :404-415 (dist) and, for runners that replay it, the sample trigger of
 * run_kitti360_bev_gen.py:218-240.  Bit-identical to the numpy expressions by construction: `cblas_dgemv64` is the
 * entry point of the cblas_dgemv (64-bit integers) of the OpenBLAS that numpy itself has loaded, so both matrix products
 * ((4,4)@(4,1) per pose, tri(n)@d) run the very kernel numpy runs; np.sum is restated as numpy's pairwise summation.
 *   pca_host_track_step      one integrate(): transform stored poses by T_new_prev, append [0,0,0], push the newest
 *                            segment, evict beyond `horizon`; returns the number of evicted frames, *path_length = the
 *                            path before the eviction (NaN while there is one pose only)
 *   pca_host_track_trigger   present index of a BEV sample, -1 if one of the driver's three conditions says no,
 *                            -2 if previous_idx is out of range (IndexError in the driver)
 *   pca_host_track_incr      tri(n) @ d into out[n_segments]
 * poses(): [len][4] doubles x, y, z, 1 (valid until the next mutating call); segments(): [n_segments].
 * ------------------------------------------------------------------------------------------------ */
typedef struct pca_host_track pca_host_track;
/* The (4,4)@(4,1) product per pose: mode 0 calls cblas_dgemv (exact by construction, ~150 ns of call overhead per pose);
 * modes 1..5 are the closed forms a dgemv kernel can reduce to for a 4-long dot product.  The binding probes them against
 * numpy on random data (pca_host_gemv4_probe) and selects one only if it agrees everywhere (pca_host_gemv4_mode). */
int pca_host_gemv4_probe(void *cblas_dgemv64, int mode, const double *T /*[n][16]*/, const double *x /*[n][4]*/, int64_t n,
                         double *y /*[n][4]*/);
int pca_host_gemv4_mode(int mode);
/* tri(n) @ d: the eviction needs its first rows, the trigger its last row and one crossing.  With blocks on, groups of 8
 * rows (from a multiple of 8) are computed on their own instead of the full n x n product; the binding turns that on only
 * after pca_host_incr_probe reproduced numpy's full product on random data. */
int pca_host_incr_probe(void *cblas_dgemv64, const double *d, int64_t n, int64_t r0, int64_t r1, double *out);
int pca_host_incr_blocks(int on);
int pca_host_track_create(pca_host_track **out, void *cblas_dgemv64);
void pca_host_track_destroy(pca_host_track *t);
int64_t pca_host_track_len(const pca_host_track *t);
int64_t pca_host_track_n_segments(const pca_host_track *t);
const double *pca_host_track_poses(const pca_host_track *t);
const double *pca_host_track_segments(const pca_host_track *t);
int pca_host_track_set(pca_host_track *t, const double *poses /*[n][3]*/, int64_t n, const double *segs, int64_t nd);
int pca_host_track_transform(pca_host_track *t, const double T[16]);
int pca_host_track_append(pca_host_track *t, const double pose[3]);
int pca_host_track_push_segment(pca_host_track *t, double *path_length);
int pca_host_track_incr(pca_host_track *t, double *out);
int64_t pca_host_track_evict_beyond(pca_host_track *t, double horizon, double path_length);
int64_t pca_host_track_step(pca_host_track *t, const double T_new_prev[16], double horizon, double *path_length);
int64_t pca_host_track_trigger(pca_host_track *t, double bev_horizon, int64_t previous_idx, double min_step);

/* ------------------------------------------------------------------------------------------------
 * Optional timing with HIP events recorded on the call's stream.  on = 1: every kernel launch is bracketed
 * (ids PCA_K_KITTI .. PCA_K_DEDUP); on = 2: only whole multi-kernel units are (PCA_K_BEV_UNIT = one
 * pca_bev_generate call, launch gaps included, without the per-kernel events in between); 0: off.  pca_profile_read synchronises, returns the accumulated time / launch count of one
 * kernel id since the last pca_profile_enable(ctx, 1) and keeps recording.  (No reference counterpart.)
 * PCA_K_BEV_SCAN / PCA_K_BEV_SCATTER are kept for the numbering only: level 1 of the rasteriser is one kernel
 * (PCA_K_BEV_BIN) since round 2 and these two never record a launch.
 * ------------------------------------------------------------------------------------------------ */
enum {
    PCA_K_KITTI = 0, PCA_K_NUSC, PCA_K_PROJECT_CAMS, PCA_K_RETRANSFORM, PCA_K_MARK_DYNAMIC,
    PCA_K_BEV_BIN, PCA_K_BEV_SCAN, PCA_K_BEV_SCATTER, PCA_K_BEV_CELLS, PCA_K_BEV_CELLS_HEAVY, PCA_K_DEDUP, PCA_K_BEV_UNIT, PCA_K_ICP,
    PCA_K_BEV_CLASS_BIN, PCA_K_BEV_CLASS_CELLS, PCA_K_BEV_ELEV_BIN, PCA_K_BEV_ELEV_CELLS,
    PCA_K_BEV_VOXEL_BIN, PCA_K_BEV_VOXEL_CELLS, PCA_K_BEV_VOXEL_RAYS, PCA_K_RENDER_ZBUFFER, PCA_K_RENDER_RESOLVE,
    PCA_K_BEV_CARVE_ENDS, PCA_K_BEV_CARVE_RAYS, PCA_K_BEV_CARVE_FLAGS, PCA_K_COUNT
};
/* The ids that follow (the first block above is closed: its length is pinned): the kernels of pca_bev_voxel_instances, then
 * the one of pca_bev_voxel_camera. */
enum {
    PCA_K_BEV_INST_INIT = PCA_K_COUNT, PCA_K_BEV_INST_MERGE, PCA_K_BEV_INST_COMPRESS, PCA_K_BEV_INST_SUMS, PCA_K_BEV_INST_OFFSETS,
    PCA_K_BEV_INST_NUMBER, PCA_K_BEV_INST_WRITE, PCA_K_BEV_INST_POINTS, PCA_K_BEV_CAMERA_RAYS, PCA_K_TOTAL
};
/* A third block (the second is closed too): the kernels of pca_voxel_pool and pca_voxel_pack. */
enum {
    PCA_K_VOXEL_POOL = PCA_K_TOTAL, PCA_K_VOXEL_PACK, PCA_K_END
};
/* A fourth block (the third is closed as well): the two kernels of pca_voxel_distance. */
enum {
    PCA_K_VOXEL_DIST_LINES = PCA_K_END, PCA_K_VOXEL_DIST_ROWS, PCA_K_LAST
};
/* A fifth block (the fourth is closed too): the seven kernels of pca_bev_instance_boxes.  The profiler's tables end here. */
enum {
    PCA_K_BEV_BOX_TABLE = PCA_K_LAST, PCA_K_BEV_BOX_COUNT, PCA_K_BEV_BOX_OFFSETS, PCA_K_BEV_BOX_SCATTER, PCA_K_BEV_BOX_EXTENTS, PCA_K_BEV_BOX_NEAR,
    PCA_K_BEV_BOX_CHOOSE, PCA_K_ALL
};
int pca_profile_enable(pca_ctx *ctx, int on);
int pca_profile_read(pca_ctx *ctx, int kernel_id, double *total_ms, int64_t *launches);

#ifdef __cplusplus
}
#endif
#endif /* PCA_H */
