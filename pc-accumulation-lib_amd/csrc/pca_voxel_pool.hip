// pca_voxel_pool.hip -- the voxel volumes of the occupancy chain (labels, seen, visible: pca_bev_voxel.hip, pca_bev_rays.hip,
// pca_bev_camera.hip) turned into what a semantic-scene-completion trainer loads: the coarser scales 1:2, 1:4 and 1:8, and the
// payloads of SemanticKITTI-SSC's files (.label, .invalid, .occluded, .bin).  Both entries read volumes: no store, no points.
//
//   voxel_pool   one launch for every requested scale, one pass over the fine volume.  A workgroup of 256 threads takes tiles of
//                POOL_TK x POOL_TR x POOL_W = 8 x 8 x 64 fine voxels (k, row, col), a grid-stride loop over the tiles.
//                1: the three inputs of the tile are loaded along col -- 16 voxels per thread, as dwords where px and the
//                   pointers allow it, else as bytes -- and folded into ONE byte per voxel in LDS: the label (0..31), or 32
//                   UNSEEN / 33 FREE, 63 for a voxel outside the volume (it counts in nothing), bit 7 = visible.
//                2: one thread per scale-2 cell (512 of them, col fastest) builds the cell's per-label counts in LDS as bytes,
//                   by read-modify-write of its own row -- a per-lane array of 32 counters indexed by the label would live in
//                   scratch -- plus one word {n_free, n_visible, n_occ}; a row is 36 bytes = 9 dwords, an odd number, so the
//                   32 lanes of a half wave that touch the same label hit 32 different banks.
//                3: the rows of the eight children are added up into the scale-4 rows (64 cells, still bytes: a count is at most
//                   64, so the four bytes of a dword are added as one u32) and those into the scale-8 rows (8 cells, u16).  The
//                   COUNTS go up the hierarchy, never a decision.
//                4: one thread per cell of each requested scale decides (occupied, smallest label among the most frequent,
//                   free / unseen, visible) and writes its bytes.  A scale is only requested where it divides px and nz, so a
//                   cell of a requested scale lies inside the volume whole or not at all.
//                The volume is 2 M voxels at 256 x 256 x 32: the launch and the latency of the first loads bound this kernel,
//                not bandwidth.
//   voxel_pack   one launch per level.  Voxel (i, j, k) lives at [k][px-1-j][i]; its place in every output is
//                t = (i px + j) nz + k (SemanticKITTI's x, y, z with z fastest).  A workgroup takes tiles of 64 columns i x CJ
//                values of j x all k, CJ = 128 / nz: the reads run along col (a wave loads 64 neighbouring bytes), the tile is
//                transposed through LDS (the u16 file value and three bits per voxel; row strides of 65 and 33 dwords), and the
//                writes run along t: per column a run of CJ nz places.  A bit stream is written 64 places at a time: the wave's
//                __ballot is eight finished bytes once each byte is turned MSB-first (bit-reverse the 64 bits, then swap the
//                bytes).  A byte belongs to the tile that holds its FIRST bit; up to seven later bits of it may lie in the next
//                tile and are then read from global memory directly, and the bits behind the last voxel are 0.  No atomics, and
//                every byte is written once.
// Out of scope: votes weighted by point counts instead of voxels; scales other than 2, 4, 8; coarse .occluded / .bin files;
// Occ3D's .npz container (its arrays are level 1's labels, seen and visible); how the fine volumes are made; banded grids above
// 1024.
#include "pca_common.h"

#define POOL_THREADS 256
#define POOL_TK 8
#define POOL_TR 8
#define POOL_W 64
#define POOL_ROW 36               // bytes of a cell's count row: 32 labels, n_free, n_visible, n_occ, one spare
#define POOL_MAX_G 2048
#define POOL_ABSENT 63
#define POOL_UNSEEN 32
#define POOL_FREE 33

struct PoolOut { uint8_t *labels, *state, *visible; };
struct alignas(16) PoolArgs {
    int px, nz, G, wide;          // wide: dword loads (px % 4 == 0 and the three pointers 4-aligned)
    int tiles_c, tiles_r, tiles;
    int occ_num, occ_den;
    const uint8_t *labels, *seen, *visible;
    PoolOut out[3];               // scale 2, 4, 8; all NULL: not requested
};

__device__ __forceinline__ uint32_t pool_code(uint32_t lab, uint32_t seen, uint32_t vis)
{
    const uint32_t c = lab < PCA_BEV_VOXEL_MAX_LABELS ? lab : (seen ? POOL_FREE : POOL_UNSEEN);
    return c | (vis ? 0x80u : 0u);
}

// One coarse cell decided from its counts (T: u8 or u16 [POOL_ROW]) and written; n = s^3 fine voxels.
template <typename T>
__device__ __forceinline__ void pool_decide(const PoolArgs &a, const PoolOut &o, const T *row, int n, int64_t at)
{
    const int n_free = row[32], n_vis = row[33], n_occ = row[34];
    int best = 0, best_n = row[0];
#pragma unroll 8
    for (int l = 1; l < PCA_BEV_VOXEL_MAX_LABELS; ++l) {
        const int c = row[l];
        if (c > best_n) { best_n = c; best = l; }
    }
    const bool occ = n_occ > 0 && (int64_t)n_occ * a.occ_den >= (int64_t)n * a.occ_num;
    if (o.labels) o.labels[at] = occ ? (uint8_t)best : (uint8_t)255;
    if (o.state) o.state[at] = occ ? 2 : (n_free > n - n_occ - n_free ? 1 : 0);
    if (o.visible) o.visible[at] = n_vis ? 1 : 0;
}

__global__ __launch_bounds__(POOL_THREADS) void voxel_pool(const PoolArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_code[POOL_TK * POOL_TR * POOL_W];
    __shared__ __attribute__((aligned(16))) uint8_t s_c2[512 * POOL_ROW];
    __shared__ __attribute__((aligned(16))) uint8_t s_c4[64 * POOL_ROW];
    __shared__ __attribute__((aligned(16))) uint16_t s_c8[8 * POOL_ROW];
    const int tid = (int)threadIdx.x, px = a.px, nz = a.nz;
    const bool want2 = a.out[0].labels || a.out[0].state || a.out[0].visible;
    const bool want4 = a.out[1].labels || a.out[1].state || a.out[1].visible;
    const bool want8 = a.out[2].labels || a.out[2].state || a.out[2].visible;

    for (int tile = (int)blockIdx.x; tile < a.tiles; tile += a.G) {
        const int tc = tile % a.tiles_c, tr = (tile / a.tiles_c) % a.tiles_r, tk = tile / (a.tiles_c * a.tiles_r);
        const int k0 = tk * POOL_TK, r0 = tr * POOL_TR, c0 = tc * POOL_W;
        // 1: 16 voxels of one (k, row) line per thread
        {
            const int line = tid >> 2, seg = (tid & 3) * 16;
            const int k = k0 + (line >> 3), r = r0 + (line & 7), c = c0 + seg;
            uint32_t w[4] = {0x3f3f3f3fu, 0x3f3f3f3fu, 0x3f3f3f3fu, 0x3f3f3f3fu};      // POOL_ABSENT
            if (k < nz && r < px && c < px) {
                const int64_t at = ((int64_t)k * px + r) * px + c;
                if (a.wide) {
                    // (px % 4 == 0 and c % 16 == 0: a dword lies inside the line whole or not at all)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        if (c + 4 * q < px) {
                            const uint32_t lab = pca_ldg(reinterpret_cast<const uint32_t *>(a.labels + at) + q);
                            const uint32_t sn = pca_ldg(reinterpret_cast<const uint32_t *>(a.seen + at) + q);
                            const uint32_t vs = a.visible ? pca_ldg(reinterpret_cast<const uint32_t *>(a.visible + at) + q) : 0u;
                            uint32_t v = 0;
#pragma unroll
                            for (int b = 0; b < 4; ++b)
                                v |= pool_code((lab >> (8 * b)) & 255u, (sn >> (8 * b)) & 255u, (vs >> (8 * b)) & 255u) << (8 * b);
                            w[q] = v;
                        }
                    }
                } else {
                    for (int e = 0; e < 16; ++e) {
                        if (c + e < px) {
                            const uint32_t code = pool_code(pca_ldg(a.labels + at + e), pca_ldg(a.seen + at + e),
                                                            a.visible ? pca_ldg(a.visible + at + e) : 0u);
                            w[e >> 2] = (w[e >> 2] & ~(255u << (8 * (e & 3)))) | (code << (8 * (e & 3)));
                        }
                    }
                }
            }
            uint32_t *dst = reinterpret_cast<uint32_t *>(s_code + line * POOL_W + seg);
            dst[0] = w[0]; dst[1] = w[1]; dst[2] = w[2]; dst[3] = w[3];
        }
        __syncthreads();
        // 2: the count rows of the scale-2 cells; cell = (kk * 4 + rr) * 32 + cc
        for (int cell = tid; cell < 512; cell += POOL_THREADS) {
            const int cc = cell & 31, rr = (cell >> 5) & 3, kk = cell >> 7;
            uint8_t *row = s_c2 + cell * POOL_ROW;
            uint32_t *row32 = reinterpret_cast<uint32_t *>(row);
#pragma unroll
            for (int q = 0; q < POOL_ROW / 4; ++q) row32[q] = 0;
            uint32_t n_free = 0, n_vis = 0, n_occ = 0;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const int line = (2 * kk + (d >> 1)) * POOL_TR + 2 * rr + (d & 1);
                const uint32_t pair = *reinterpret_cast<const uint16_t *>(s_code + line * POOL_W + 2 * cc);
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const uint32_t code = (pair >> (8 * h)) & 255u, c = code & 63u;
                    n_vis += code >> 7;
                    n_free += c == POOL_FREE ? 1u : 0u;
                    if (c < PCA_BEV_VOXEL_MAX_LABELS) { ++n_occ; row[c] = (uint8_t)(row[c] + 1); }
                }
            }
            row32[8] = n_free | (n_vis << 8) | (n_occ << 16);
            if (want2) {
                const int k = (k0 >> 1) + kk, r = (r0 >> 1) + rr, c = (c0 >> 1) + cc, p2 = px >> 1;
                if (2 * k < nz && 2 * r < px && 2 * c < px) pool_decide(a, a.out[0], row, 8, ((int64_t)k * p2 + r) * p2 + c);
            }
        }
        if (want4 || want8) {
            __syncthreads();
            // 3a: scale-4 rows, a dword = four byte counters (no byte passes 64); cell = (kk * 2 + rr) * 16 + cc
            for (int task = tid; task < 64 * (POOL_ROW / 4); task += POOL_THREADS) {
                const int cell = task / (POOL_ROW / 4), q = task % (POOL_ROW / 4);
                const int cc = cell & 15, rr = (cell >> 4) & 1, kk = cell >> 5;
                uint32_t sum = 0;
#pragma unroll
                for (int d = 0; d < 8; ++d) {
                    const int child = ((2 * kk + (d >> 2)) * 4 + 2 * rr + ((d >> 1) & 1)) * 32 + 2 * cc + (d & 1);
                    sum += reinterpret_cast<const uint32_t *>(s_c2 + child * POOL_ROW)[q];
                }
                reinterpret_cast<uint32_t *>(s_c4 + cell * POOL_ROW)[q] = sum;
            }
            __syncthreads();
            if (want4 && tid < 64) {
                const int cc = tid & 15, rr = (tid >> 4) & 1, kk = tid >> 5;
                const int k = (k0 >> 2) + kk, r = (r0 >> 2) + rr, c = (c0 >> 2) + cc, p4 = px >> 2;
                if (4 * k < nz && 4 * r < px && 4 * c < px)
                    pool_decide(a, a.out[1], s_c4 + tid * POOL_ROW, 64, ((int64_t)k * p4 + r) * p4 + c);
            }
            if (want8) {
                // 3b: scale-8 rows (u16: up to 512); cell = cc, the tile is one cell high and deep
                for (int task = tid; task < 8 * POOL_ROW; task += POOL_THREADS) {
                    const int cc = task / POOL_ROW, e = task % POOL_ROW;
                    uint32_t sum = 0;
#pragma unroll
                    for (int d = 0; d < 8; ++d) {
                        const int child = ((d >> 2) * 2 + ((d >> 1) & 1)) * 16 + 2 * cc + (d & 1);
                        sum += s_c4[child * POOL_ROW + e];
                    }
                    s_c8[cc * POOL_ROW + e] = (uint16_t)sum;
                }
                __syncthreads();
                if (tid < 8) {
                    const int k = k0 >> 3, r = r0 >> 3, c = (c0 >> 3) + tid, p8 = px >> 3;
                    if (8 * c < px) pool_decide(a, a.out[2], s_c8 + tid * POOL_ROW, 512, ((int64_t)k * p8 + r) * p8 + c);
                }
            }
        }
        __syncthreads();          // (the next tile overwrites what this one's last readers read)
    }
}

// ------------------------------------------------------------------------------------------------------------------- pack
#define PACK_THREADS 256
#define PACK_CI 64                // columns i of a tile
#define PACK_U 128                // places (j, k) of a column in a tile, at most: CJ = PACK_U / nz values of j
#define PACK_VAL_STRIDE 130       // u16: 65 dwords a column
#define PACK_BIT_STRIDE 132       // u8: 33 dwords a column
#define PACK_MAX_G 2048
#define PACK_INVALID 1u
#define PACK_OCCLUDED 2u
#define PACK_BIN 4u

struct alignas(16) PackArgs {
    int px, nz, G, cj;
    int tiles_i, tiles;
    const uint8_t *labels, *seen, *visible, *input_occ;
    uint16_t *label_out;
    uint8_t *invalid_bits, *occluded_bits, *bin_bits;
    uint16_t map[PCA_BEV_VOXEL_MAX_LABELS + 1];       // [32] = empty_value
};

// the three bits of the voxel at `at` (bytes of inputs that are absent read as 0 and their stream is not written)
__device__ __forceinline__ uint32_t pack_bits(const PackArgs &a, uint32_t lab, int64_t at)
{
    const bool occ = lab < PCA_BEV_VOXEL_MAX_LABELS;
    uint32_t b = 0;
    if (a.seen && !occ && pca_ldg(a.seen + at) == 0) b |= PACK_INVALID;
    if (a.visible && pca_ldg(a.visible + at) == 0) b |= PACK_OCCLUDED;
    if (a.input_occ && pca_ldg(a.input_occ + at) != 0) b |= PACK_BIN;
    return b;
}

// the wave's 64 places as eight bytes of the stream: lane 8 q + b is bit 7 - b of byte q
__device__ __forceinline__ void pack_store(uint8_t *dst, bool bit, int64_t first_byte, int n_bytes, int lane)
{
    const uint64_t m = __builtin_bswap64(__builtin_bitreverse64(__ballot(bit)));
    if (dst && lane < n_bytes) dst[first_byte + lane] = (uint8_t)(m >> (8 * lane));
}

__global__ __launch_bounds__(PACK_THREADS) void voxel_pack(const PackArgs a)
{
    __shared__ uint16_t s_val[PACK_CI * PACK_VAL_STRIDE];
    __shared__ uint8_t s_bit[PACK_CI * PACK_BIT_STRIDE];
    __shared__ uint16_t s_map[PCA_BEV_VOXEL_MAX_LABELS + 1];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, px = a.px, nz = a.nz;
    const int64_t col_places = (int64_t)px * nz, total = col_places * px;
    const bool want_bits = a.invalid_bits || a.occluded_bits || a.bin_bits;
    if (tid <= PCA_BEV_VOXEL_MAX_LABELS) s_map[tid] = a.map[tid];
    __syncthreads();

    for (int tile = (int)blockIdx.x; tile < a.tiles; tile += a.G) {
        const int i0 = (tile % a.tiles_i) * PACK_CI, j0 = (tile / a.tiles_i) * a.cj;
        const int j_end = j0 + a.cj < px ? j0 + a.cj : px, run = (j_end - j0) * nz;       // run <= PACK_U
        // in: lane = column, the waves share the places of the run
        if (i0 + lane < px) {
            for (int u = wave; u < run; u += PACK_THREADS / 64) {
                const int j = j0 + u / nz, k = u % nz;
                const int64_t at = ((int64_t)k * px + (px - 1 - j)) * px + i0 + lane;
                const uint32_t lab = pca_ldg(a.labels + at);
                s_val[lane * PACK_VAL_STRIDE + u] = s_map[lab < PCA_BEV_VOXEL_MAX_LABELS ? lab : PCA_BEV_VOXEL_MAX_LABELS];
                if (want_bits) s_bit[lane * PACK_BIT_STRIDE + u] = (uint8_t)pack_bits(a, lab, at);
            }
        }
        __syncthreads();
        // out: a wave per column, lane = place
        for (int il = wave; il < PACK_CI && i0 + il < px; il += PACK_THREADS / 64) {
            const int64_t t_lo = ((int64_t)(i0 + il) * px + j0) * nz, t_hi = t_lo + run;
            if (a.label_out)
                for (int u = lane; u < run; u += 64) a.label_out[t_lo + u] = s_val[il * PACK_VAL_STRIDE + u];
            if (want_bits) {
                // the bytes whose first bit lies in [t_lo, t_hi)
                for (int64_t base = (t_lo + 7) & ~7ll; base < t_hi; base += 64) {
                    const int64_t t = base + lane;
                    uint32_t b = 0;
                    if (t < t_hi) {
                        b = s_bit[il * PACK_BIT_STRIDE + (int)(t - t_lo)];
                    } else if (t < total) {       // the tail of a byte this tile owns: at most seven places of the next tile
                        const int i = (int)(t / col_places), rem = (int)(t - (int64_t)i * col_places);
                        const int j = rem / nz, k = rem % nz;
                        const int64_t at = ((int64_t)k * px + (px - 1 - j)) * px + i;
                        b = pack_bits(a, pca_ldg(a.labels + at), at);
                    }
                    const int64_t left = (t_hi - base + 7) >> 3;
                    const int n_bytes = left < 8 ? (int)left : 8;
                    pack_store(a.invalid_bits, b & PACK_INVALID, base >> 3, n_bytes, lane);
                    pack_store(a.occluded_bits, b & PACK_OCCLUDED, base >> 3, n_bytes, lane);
                    pack_store(a.bin_bits, b & PACK_BIN, base >> 3, n_bytes, lane);
                }
            }
        }
        __syncthreads();
    }
}

static int ssc_shape_check(pca_ctx *ctx, const std::string &w, int px, int nz)
{
    if (px < 1 || px > 1024) { ctx->err = w + ": px must be in 1..1024"; return -1; }
    if (nz < 1 || nz > 32) { ctx->err = w + ": nz must be in 1..32"; return -1; }
    return 0;
}

extern "C" {

int pca_voxel_pool(pca_ctx *ctx, int px, int nz, const uint8_t *labels, const uint8_t *seen, const uint8_t *visible,
                   int occ_num, int occ_den, const pca_voxel_pool_level *levels, int n_levels, void *stream)
{
    if (!ctx) return -1;
    hipStream_t s = (hipStream_t)stream;
    const std::string w("voxel pool");
    // every check comes before the launch
    if (ssc_shape_check(ctx, w, px, nz)) return -1;
    if (!labels) { ctx->err = w + ": labels must not be NULL"; return -1; }
    if (!seen) { ctx->err = w + ": seen must not be NULL"; return -1; }
    if (occ_den < 1 || occ_num < 0 || occ_num > occ_den) { ctx->err = w + ": occ_den must be >= 1 and occ_num in 0..occ_den"; return -1; }
    if (!levels || n_levels < 1 || n_levels > 3) { ctx->err = w + ": levels must hold 1 to 3 descriptors"; return -1; }
    PoolArgs A;
    for (int q = 0; q < 3; ++q) A.out[q] = PoolOut{nullptr, nullptr, nullptr};
    for (int n = 0; n < n_levels; ++n) {
        const pca_voxel_pool_level &lv = levels[n];
        if (lv.scale != 2 && lv.scale != 4 && lv.scale != 8) { ctx->err = w + ": scale must be 2, 4 or 8"; return -1; }
        const int q = lv.scale == 2 ? 0 : (lv.scale == 4 ? 1 : 2);
        if (A.out[q].labels || A.out[q].state || A.out[q].visible) { ctx->err = w + ": a scale must not be requested twice"; return -1; }
        if (px % lv.scale || nz % lv.scale) { ctx->err = w + ": px and nz must be multiples of every requested scale"; return -1; }
        if (!lv.labels && !lv.state && !lv.visible) { ctx->err = w + ": a level needs at least one output"; return -1; }
        if (lv.visible && !visible) { ctx->err = w + ": a visible output needs the visible input"; return -1; }
        A.out[q] = PoolOut{lv.labels, lv.state, lv.visible};
    }
    A.px = px; A.nz = nz;
    A.occ_num = occ_num; A.occ_den = occ_den;
    A.labels = labels; A.seen = seen; A.visible = visible;
    A.wide = px % 4 == 0 && (((uintptr_t)labels | (uintptr_t)seen | (uintptr_t)visible) & 3) == 0;
    A.tiles_c = (px + POOL_W - 1) / POOL_W;
    A.tiles_r = (px + POOL_TR - 1) / POOL_TR;
    A.tiles = A.tiles_c * A.tiles_r * ((nz + POOL_TK - 1) / POOL_TK);      // at most 16 * 128 * 4
    // PCA_VOXEL_POOL_G: a cap on the workgroups, read on every call (tests send a workgroup round its loop again)
    const int max_g = (int)pca_env_int("PCA_VOXEL_POOL_G", POOL_MAX_G, 1, POOL_MAX_G);
    A.G = A.tiles < max_g ? A.tiles : max_g;
    PCA_CHECK(ctx, hipSetDevice(ctx->device));
    const PoolArgs &args = A;
    PCA_LAUNCH(ctx, PCA_K_VOXEL_POOL, voxel_pool, dim3(args.G), dim3(POOL_THREADS), s, args);
    PCA_CHECK(ctx, hipGetLastError());
    return 0;
}

int pca_voxel_pack(pca_ctx *ctx, int px, int nz, const uint8_t *labels, const uint8_t *seen, const uint8_t *visible,
                   const uint8_t *input_occ, const uint16_t *label_map, uint16_t empty_value, uint16_t *label_out,
                   uint8_t *invalid_bits, uint8_t *occluded_bits, uint8_t *bin_bits, void *stream)
{
    if (!ctx) return -1;
    hipStream_t s = (hipStream_t)stream;
    const std::string w("voxel pack");
    if (ssc_shape_check(ctx, w, px, nz)) return -1;
    if (!labels) { ctx->err = w + ": labels must not be NULL"; return -1; }
    if (!label_out && !invalid_bits && !occluded_bits && !bin_bits) { ctx->err = w + ": at least one output is needed"; return -1; }
    if (label_out && !label_map) { ctx->err = w + ": label_out needs label_map"; return -1; }
    if (invalid_bits && !seen) { ctx->err = w + ": invalid_bits needs seen"; return -1; }
    if (occluded_bits && !visible) { ctx->err = w + ": occluded_bits needs visible"; return -1; }
    if (bin_bits && !input_occ) { ctx->err = w + ": bin_bits needs input_occ"; return -1; }
    PackArgs A;
    A.px = px; A.nz = nz;
    A.cj = PACK_U / nz;                                                      // >= 4
    A.tiles_i = (px + PACK_CI - 1) / PACK_CI;
    A.tiles = A.tiles_i * ((px + A.cj - 1) / A.cj);                          // at most 16 * 256
    const int max_g = (int)pca_env_int("PCA_VOXEL_PACK_G", PACK_MAX_G, 1, PACK_MAX_G);
    A.G = A.tiles < max_g ? A.tiles : max_g;
    A.labels = labels;
    // (an input whose stream is not asked for is not read)
    A.seen = invalid_bits ? seen : nullptr;
    A.visible = occluded_bits ? visible : nullptr;
    A.input_occ = bin_bits ? input_occ : nullptr;
    A.label_out = label_out; A.invalid_bits = invalid_bits; A.occluded_bits = occluded_bits; A.bin_bits = bin_bits;
    for (int l = 0; l < PCA_BEV_VOXEL_MAX_LABELS; ++l) A.map[l] = label_map ? label_map[l] : 0;
    A.map[PCA_BEV_VOXEL_MAX_LABELS] = empty_value;
    PCA_CHECK(ctx, hipSetDevice(ctx->device));
    const PackArgs &args = A;
    PCA_LAUNCH(ctx, PCA_K_VOXEL_PACK, voxel_pack, dim3(args.G), dim3(PACK_THREADS), s, args);
    PCA_CHECK(ctx, hipGetLastError());
    return 0;
}

}  // extern "C"
