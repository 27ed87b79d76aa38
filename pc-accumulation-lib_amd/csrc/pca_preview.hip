// pca_preview.hip -- KP: the preview sheet of a BEV sample as a PNG made on the device (include/pca.h: pca_preview_sheets,
// pca_adler32_chunks, pca_host_adler32_combine, pca_host_png_assemble).
//
// The drivers write a viz_XXX.png beside every sample (run_kitti360_bev_gen.py:267-270 of the reference) from a matplotlib
// figure per sample.  Here the picture is a sheet of 3 x 5 panels (sets x road, intensity, rgb, dynamic, elevation) straight
// from the fp16 planes, with the trajectories drawn over every panel of their set, and what leaves the device is the PNG's
// zlib stream: the scanlines are filtered here, cut into chunks, compressed by pca_deflate_chunks[_dyn] and summed here.
//   preview_overlay   one workgroup per polyline, a lane per segment (a wave per long segment, a lane per step): ORs the
//                     covered cells into a bit mask per (sample, set), px * px bits -- the overlay is the same on the five
//                     panels of a row, and a scanline can only be filtered once it is known.
//   preview_rows      one workgroup per scanline: composes the row's pixels into LDS (with the Up filter: minus the row
//                     above, which the lane computes too), then stores it as whole dwords of filtered bytes with a byte
//                     head and tail -- a row is 1 + 15 px bytes long, so rows never start on a dword.
//   adler32_chunks    one workgroup per chunk: sum(d) and sum((n - pos) d) are sums over independent bytes, so lanes stride
//                     over aligned dwords; a lane's partial sums fit 32 bits and are reduced mod 65521 before they meet.
#include "pca_common.h"

#define PV_BLK 256
#define PV_NW (PV_BLK / PCA_WAVE)
#define PV_PANELS 5
#define PV_PAD 8                                       // zero bytes in front of the row's pixels in LDS: the Sub filter's left neighbours
#define PV_ADLER 65521u
static_assert(sizeof(pca_preview_polyline) == 16, "the polyline table is read in 16-byte records");

struct PvRanges { float lo[4], scale[4]; };            // road, intensity, dynamic, elevation

__host__ __device__ static inline int64_t pv_mask_words(int64_t px) { return (px * px + 31) / 32; }

// ---- pixels
typedef uint16_t pv_u16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float pv_f16(uint16_t h) { return __half2float(__ushort_as_half(h)); }

// LUT index of a scalar value: clamp(floor((v - lo) * scale), 0, 255); NaN -> 0
__device__ __forceinline__ uint32_t pv_index(float v, float lo, float scale)
{
    const float t = floorf((v - lo) * scale);
    return t >= 255.0f ? 255u : (t > 0.0f ? (uint32_t)t : 0u);
}
// byte of a colour channel: floor(min(max(v, 0), 1) * 255 + 0.5); NaN -> 0
__device__ __forceinline__ uint32_t pv_channel(float v)
{
    const float c = v > 0.0f ? (v < 1.0f ? v : 1.0f) : 0.0f;
    return (uint32_t)floorf(c * 255.0f + 0.5f);
}

// N pixels (r | g << 8 | b << 16) of image row R of the sheet from column q of panel c on; planes: the sample's [21][px][px].
// lo, scale: the range of a scalar panel (c != 2).  N == 4 needs px % 4 == 0 and q % 4 == 0: the loads are 8 bytes wide,
// the four mask bits lie in one word.
template <int N>
__device__ __forceinline__ void pv_pixels(const uint16_t *__restrict__ planes, const uint32_t *__restrict__ mask, const uint32_t *lut,
                                          float lo, float scale, int px, int R, int c, int q, uint32_t (&rgb)[N])
{
    const int s = R / px, r = R - s * px;
    const size_t cell = (size_t)px * px, at = (size_t)r * px + q;
    const uint16_t *set = planes + (size_t)(7 * s) * cell;
    uint16_t h[3][N] = {};
    const int first = c < 2 ? c : (c == 2 ? 2 : c + 2), n_planes = c == 2 ? 3 : 1;      // plane of the set the panel starts at
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (k >= n_planes) continue;
        const uint16_t *p = set + (size_t)(first + k) * cell + at;
        if constexpr (N == 4) {
            const pv_u16x4 v = pca_ldg(reinterpret_cast<const pv_u16x4 *>(p));
            h[k][0] = v.x; h[k][1] = v.y; h[k][2] = v.z; h[k][3] = v.w;
        } else {
            h[k][0] = pca_ldg(p);
        }
    }
    const size_t bit = (size_t)s * 32 * pv_mask_words(px) + at;
    const uint32_t over = pca_ldg(mask + (bit >> 5)) >> (bit & 31);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        uint32_t v;
        if (c == 2) v = pv_channel(pv_f16(h[0][i])) | (pv_channel(pv_f16(h[1][i])) << 8) | (pv_channel(pv_f16(h[2][i])) << 16);
        else v = lut[pv_index(pv_f16(h[0][i]), lo, scale)];
        rgb[i] = (over >> i) & 1u ? 0x0000ffu : v;
    }
}

// a - b in every byte
__device__ __forceinline__ uint32_t pv_sub_bytes(uint32_t a, uint32_t b)
{
    return ((a | 0x80808080u) - (b & 0x7f7f7f7fu)) ^ ((a ^ ~b) & 0x80808080u);
}
// the four LDS bytes from byte `at` on, any alignment (two aligned dwords)
__device__ __forceinline__ uint32_t pv_lds_u32(const uint32_t *img, int at)
{
    const uint32_t lo = img[at >> 2], sh = 8u * (at & 3);
    return sh ? (lo >> sh) | (img[(at >> 2) + 1] << (32u - sh)) : lo;
}

// LDS: the LUT as 256 packed colours, then the row: PV_PAD zero bytes, 15 px bytes of pixels, zeros up to a dword and one more
__host__ __device__ static inline int pv_row_dwords(int px) { return (PV_PAD + 15 * px + 3) / 4 + 2; }

template <int N>
__global__ __launch_bounds__(PV_BLK) void preview_rows(const uint16_t *__restrict__ planes, const uint32_t *__restrict__ mask,
                                                       const uint8_t *__restrict__ lut_g, PvRanges rg, int px, int filter,
                                                       uint8_t *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t pv_lds[];
    uint32_t *lut = pv_lds, *img = pv_lds + 256;
    const int tid = threadIdx.x;
    const int rows = 3 * px, k = blockIdx.x / rows, R = blockIdx.x - k * rows;
    const int64_t row_bytes = 1 + 15 * (int64_t)px;
    planes += (size_t)k * 21 * px * px;
    mask += (size_t)k * 3 * pv_mask_words(px);

    lut[tid] = (uint32_t)pca_ldg(lut_g + 3 * tid) | ((uint32_t)pca_ldg(lut_g + 3 * tid + 1) << 8) | ((uint32_t)pca_ldg(lut_g + 3 * tid + 2) << 16);
    const int row_dw = pv_row_dwords(px);
    if (tid < PV_PAD / 4) img[tid] = 0;
    if (tid >= PV_BLK - 3) img[row_dw - (PV_BLK - tid)] = 0;          // the last three dwords: what the pixels leave of them stays zero
    __syncthreads();

    // ---- compose: N pixels per lane and step, 3 N bytes at LDS byte PV_PAD + 3 p
    const bool up = filter == 2 && R > 0;
    const int per_panel = px / N;
    uint8_t *img_b = reinterpret_cast<uint8_t *>(img);
    for (int w = tid; w < PV_PANELS * per_panel; w += PV_BLK) {
        const int c = w / per_panel, q = (w - c * per_panel) * N;
        // (a select chain: a lane-indexed read of the kernel's arguments would go through scratch)
        const float lo = c == 0 ? rg.lo[0] : c == 1 ? rg.lo[1] : c == 3 ? rg.lo[2] : rg.lo[3];
        const float scale = c == 0 ? rg.scale[0] : c == 1 ? rg.scale[1] : c == 3 ? rg.scale[2] : rg.scale[3];
        uint32_t cur[N];
        pv_pixels<N>(planes, mask, lut, lo, scale, px, R, c, q, cur);
        if (up) {
            uint32_t above[N];
            pv_pixels<N>(planes, mask, lut, lo, scale, px, R - 1, c, q, above);
#pragma unroll
            for (int i = 0; i < N; ++i) cur[i] = pv_sub_bytes(cur[i], above[i]) & 0xffffffu;
        }
        const int at = PV_PAD + 3 * (c * px + q);
        if constexpr (N == 4) {                                       // 12 bytes on a dword
            uint32_t *d = img + (at >> 2);
            d[0] = cur[0] | (cur[1] << 24);
            d[1] = (cur[1] >> 8) | (cur[2] << 16);
            d[2] = (cur[2] >> 16) | (cur[3] << 8);
        } else {
            img_b[at] = (uint8_t)cur[0]; img_b[at + 1] = (uint8_t)(cur[0] >> 8); img_b[at + 2] = (uint8_t)(cur[0] >> 16);
        }
    }
    __syncthreads();

    // ---- store: byte j of the row is the filter type (j == 0) or pixel byte j - 1, with Sub minus pixel byte j - 4 (zero
    // left of the row).  In LDS these are bytes j + 7 and j + 4.  Whole aligned dwords of the output, the bytes before the first and behind the last on their own: the
    // dwords at a row's ends are shared with the neighbouring rows, which other workgroups write.
    uint8_t *dst = out + ((size_t)k * rows + R) * row_bytes;
    const bool sub = filter == 1;
    auto row_u32 = [&](int j) -> uint32_t {                           // row bytes j >= 0 .. j + 3 (those behind the row: unspecified)
        uint32_t v = pv_lds_u32(img, j + PV_PAD - 1);
        if (sub) v = pv_sub_bytes(v, pv_lds_u32(img, j + PV_PAD - 4));
        return j == 0 ? (v & ~0xffu) | (uint32_t)filter : v;
    };
    int head = (int)((0u - reinterpret_cast<uintptr_t>(dst)) & 3u);
    head = head < row_bytes ? head : (int)row_bytes;
    const int body = (int)((row_bytes - head) >> 2), done = head + 4 * body, tail = (int)row_bytes - done;
    if (tid < head) dst[tid] = (uint8_t)(row_u32(0) >> (8 * tid));
    if (tid >= 64 && tid - 64 < tail) dst[done + tid - 64] = (uint8_t)(row_u32(done) >> (8 * (tid - 64)));
    uint32_t *dst_w = reinterpret_cast<uint32_t *>(dst + head);
    for (int d = tid; d < body; d += PV_BLK) dst_w[d] = row_u32(head + 4 * d);
}

// floor(a / b), b > 0
__device__ __forceinline__ int64_t pv_floordiv(int64_t a, int64_t b)
{
    const int64_t q = a / b;
    return a - q * b < 0 ? q - 1 : q;
}

// Vertices are taken as they are up to +-2^29 (the host clamps there): differences and step counts fit 32 bits, 2 s d + n
// stays below 2^62.
#define PV_COORD_MAX (1 << 29)
#define PV_SHORT 8                                     // steps a lane walks on its own; a longer segment is walked by its wave

struct PvSegment { int x0, y0, dx, dy, n, s_lo, s_hi; };      // the steps s_lo .. s_hi are those whose cell can lie in the grid

// step s of a segment into the mask m of its (sample, set): bit (px - 1 - y) px + x
__device__ __forceinline__ void pv_plot(const PvSegment &g, int s, int px, uint32_t *m)
{
    int64_t x = g.x0, y = g.y0;
    if (g.n > 0) {
        x += pv_floordiv(2 * (int64_t)s * g.dx + g.n, 2 * (int64_t)g.n);
        y += pv_floordiv(2 * (int64_t)s * g.dy + g.n, 2 * (int64_t)g.n);
    }
    if (x < 0 || x >= px || y < 0 || y >= px) return;
    const int64_t bit = (px - 1 - y) * px + x;
    atomicOr(&m[bit >> 5], 1u << (bit & 31));
}

// One workgroup per polyline, a lane per segment, 256 segments at a time.  Trajectories are mostly vertices a cell or two
// apart: a lane walks the few steps of its segment itself.  A segment of more steps is handed to the lane's wave, a lane per
// step.
__global__ __launch_bounds__(PV_BLK) void preview_overlay(const int32_t *__restrict__ verts, int64_t n_verts,
                                                          const pca_preview_polyline *__restrict__ lines, int k, int px,
                                                          uint32_t *__restrict__ mask)
{
    const int tid = threadIdx.x, lane = tid & 63;
    const int sample = pca_sload(&lines[blockIdx.x].sample), set = pca_sload(&lines[blockIdx.x].set);
    const int64_t first = pca_sload(&lines[blockIdx.x].first), count = pca_sload(&lines[blockIdx.x].count);
    if (sample < 0 || sample >= k || set < 0 || set >= 3 || first < 0 || count <= 0 || first + count > n_verts) return;
    uint32_t *m = mask + ((size_t)sample * 3 + set) * pv_mask_words(px);
    auto clampc = [](int v) { return v < -PV_COORD_MAX ? -PV_COORD_MAX : (v > PV_COORD_MAX ? PV_COORD_MAX : v); };
    const int32_t *v = verts + 2 * first;
    const int64_t n_seg = count > 1 ? count - 1 : 1;                // a polyline of one vertex: one segment of no length
    for (int64_t e0 = 0; e0 < n_seg; e0 += PV_BLK) {
        const int64_t e = e0 + tid;
        PvSegment g = {0, 0, 0, 0, 0, 0, -1};
        if (e < n_seg) {
            g.x0 = clampc(pca_ldg(v + 2 * e));
            g.y0 = clampc(pca_ldg(v + 2 * e + 1));
            if (count > 1) {
                g.dx = clampc(pca_ldg(v + 2 * e + 2)) - g.x0;
                g.dy = clampc(pca_ldg(v + 2 * e + 3)) - g.y0;
            }
            const int ax = g.dx < 0 ? -g.dx : g.dx, ay = g.dy < 0 ? -g.dy : g.dy;
            g.n = ax > ay ? ax : ay;
            g.s_lo = 0;
            g.s_hi = 0;
            if (g.n > 0) {
                // along its longer axis the segment moves one cell per step, exactly (d = +-n: floordiv(+-2 s n + n, 2 n) = +-s),
                // so the steps whose cell can lie in the grid are a range that is known without walking the others
                const int m0 = ax >= ay ? g.x0 : g.y0, md = ax >= ay ? g.dx : g.dy;
                const int64_t lo = md > 0 ? -(int64_t)m0 : (int64_t)m0 - (px - 1), hi = md > 0 ? (int64_t)px - 1 - m0 : m0;
                g.s_lo = (int)(lo < 0 ? 0 : (lo > g.n ? g.n : lo));
                g.s_hi = (int)(hi > g.n ? g.n : (hi < -1 ? -1 : hi));
            }
        }
        const int steps = g.s_hi - g.s_lo + 1;                      // <= 0: nothing of the segment is in the grid
        if (steps > 0 && steps <= PV_SHORT)
            for (int s = g.s_lo; s <= g.s_hi; ++s) pv_plot(g, s, px, m);
        for (uint64_t todo = __ballot(steps > PV_SHORT); todo; todo &= todo - 1) {      // (uniform in the wave: every lane comes along)
            const int src = __builtin_ctzll(todo);
            PvSegment w;
            w.x0 = __shfl(g.x0, src); w.y0 = __shfl(g.y0, src); w.dx = __shfl(g.dx, src); w.dy = __shfl(g.dy, src);
            w.n = __shfl(g.n, src); w.s_lo = __shfl(g.s_lo, src); w.s_hi = __shfl(g.s_hi, src);
            for (int s = w.s_lo + lane; s <= w.s_hi; s += PCA_WAVE) pv_plot(w, s, px, m);
        }
    }
}

__global__ __launch_bounds__(PV_BLK) void adler32_chunks(const uint8_t *__restrict__ src, const pca_deflate_chunk *__restrict__ table,
                                                         uint32_t *__restrict__ out)
{
    __shared__ uint32_t part[2][PV_NW];
    const int tid = threadIdx.x, c = blockIdx.x;
    const int64_t off = pca_sload(&table[c].offset);
    int n = pca_sload(&table[c].length);
    n = n < 0 ? 0 : (n > PCA_DEFLATE_CHUNK_MAX ? PCA_DEFLATE_CHUNK_MAX : n);
    const uint8_t *base = src + off;
    const int sh = (int)(reinterpret_cast<uintptr_t>(base) & 3u);
    // aligned dwords that hold at least one byte of the chunk: none of them can lie on a page the chunk does not touch
    const uint32_t *a = reinterpret_cast<const uint32_t *>(base - sh);
    const int K = n > 0 ? (sh + n + 3) >> 2 : 0;
    // a lane sees at most 33 dwords: sum(d) <= 132 * 255, sum((n - pos) d) <= 132 * 32768 * 255 < 2^32
    uint32_t s1 = 0, s2 = 0;
    for (int D = tid; D < K; D += PV_BLK) {
        const uint32_t w = pca_ldg(a + D);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int pos = 4 * D + t - sh;
            const uint32_t d = pos >= 0 && pos < n ? (w >> (8 * t)) & 255u : 0u;
            s1 += d;
            s2 += (uint32_t)(n - pos) * d;
        }
    }
    s1 = wave_reduce_add(s1);                                      // <= 32768 * 255
    s2 = wave_reduce_add(s2 % PV_ADLER);
    if ((tid & 63) == 0) { part[0][tid >> 6] = s1; part[1][tid >> 6] = s2; }
    __syncthreads();
    if (tid == 0) {
        uint32_t A = 1, B = (uint32_t)n;                           // the initial 1 is summed n times into B
#pragma unroll
        for (int w = 0; w < PV_NW; ++w) { A += part[0][w]; B += part[1][w]; }
        out[c] = ((B % PV_ADLER) << 16) | (A % PV_ADLER);
    }
}

// internal (pca_host.hip): the side stream of pca_host_d2h_async
int pca_side_begin(pca_ctx *ctx, hipStream_t after);
int pca_side_ticket(pca_ctx *ctx);

extern "C" int64_t pca_preview_stream_bytes(int32_t px)
{
    if (px < 1 || px > PCA_PREVIEW_MAX_PX) return -1;
    return (1 + 15 * (int64_t)px) * 3 * px;
}

extern "C" int64_t pca_preview_workspace_bytes(int32_t k, int32_t px)
{
    if (k < 0 || px < 1 || px > PCA_PREVIEW_MAX_PX) return -1;
    return 256 + pca_align256(4 * 3 * (int64_t)k * pv_mask_words(px));
}

extern "C" int pca_preview_sheets(pca_ctx *ctx, const void *planes, int32_t k, int32_t px, const int32_t *verts, int64_t n_verts,
                                  const pca_preview_polyline *polylines, int32_t n_polylines, const uint8_t *lut, const float *ranges,
                                  int32_t filter, void *out_stream, void *workspace, void *stream)
{
    if (!ctx) return -1;
    if (k < 0 || px < 1 || px > PCA_PREVIEW_MAX_PX || filter < 0 || filter > 2 || n_polylines < 0 || n_verts < 0 || !ranges ||
        (int64_t)k * 3 * px > INT32_MAX || (k > 0 && (!planes || !lut || !out_stream || !workspace)) ||
        (n_polylines > 0 && (!polylines || (n_verts > 0 && !verts)))) {
        ctx->err = "preview_sheets: bad arguments";
        return -1;
    }
    PCA_CHECK(ctx, hipSetDevice(ctx->device));
    if (pca_side_begin(ctx, (hipStream_t)stream)) return -1;
    hipStream_t s = ctx->d2h_stream;
    if (k > 0) {
        uint32_t *mask = reinterpret_cast<uint32_t *>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
        PCA_CHECK(ctx, hipMemsetAsync(mask, 0, (size_t)(4 * 3 * (int64_t)k * pv_mask_words(px)), s));
        if (n_polylines > 0)
            hipLaunchKernelGGL(preview_overlay, dim3((unsigned)n_polylines), dim3(PV_BLK), 0, s, verts, n_verts, polylines, (int)k, (int)px, mask);
        PvRanges rg;
        for (int i = 0; i < 4; ++i) { rg.lo[i] = ranges[2 * i]; rg.scale[i] = ranges[2 * i + 1]; }
        const size_t shm = 4 * (size_t)(256 + pv_row_dwords(px));
        const dim3 grid((unsigned)(k * 3 * px));
        if (px % 4 == 0 && (reinterpret_cast<uintptr_t>(planes) & 7u) == 0)      // (a view at an odd element: the narrow loads)
            hipLaunchKernelGGL(preview_rows<4>, grid, dim3(PV_BLK), shm, s, static_cast<const uint16_t *>(planes), mask, lut, rg, (int)px,
                               (int)filter, static_cast<uint8_t *>(out_stream));
        else
            hipLaunchKernelGGL(preview_rows<1>, grid, dim3(PV_BLK), shm, s, static_cast<const uint16_t *>(planes), mask, lut, rg, (int)px,
                               (int)filter, static_cast<uint8_t *>(out_stream));
        PCA_CHECK(ctx, hipGetLastError());
    }
    return pca_side_ticket(ctx);
}

extern "C" int pca_adler32_chunks(pca_ctx *ctx, const void *src, const pca_deflate_chunk *chunk_table, int64_t n_chunks, uint32_t *out,
                                  void *stream)
{
    if (!ctx) return -1;
    if (n_chunks < 0 || n_chunks > PCA_DEFLATE_MAX_CHUNKS || (n_chunks > 0 && (!src || !chunk_table || !out))) {
        ctx->err = "adler32_chunks: bad arguments";
        return -1;
    }
    PCA_CHECK(ctx, hipSetDevice(ctx->device));
    if (pca_side_begin(ctx, (hipStream_t)stream)) return -1;
    if (n_chunks > 0) {
        hipLaunchKernelGGL(adler32_chunks, dim3((unsigned)n_chunks), dim3(PV_BLK), 0, ctx->d2h_stream, static_cast<const uint8_t *>(src),
                           chunk_table, out);
        PCA_CHECK(ctx, hipGetLastError());
    }
    return pca_side_ticket(ctx);
}

// ---- host: Adler-32 of concatenations, the PNG container
extern "C" uint32_t pca_host_adler32_combine(uint32_t adler_a, uint32_t adler_b, int64_t len_b)
{
    if (len_b < 0) return 0;
    const uint32_t rem = (uint32_t)(len_b % PV_ADLER);
    uint32_t s1 = adler_a & 0xffffu, s2 = (uint32_t)(((uint64_t)rem * s1) % PV_ADLER);
    s1 += (adler_b & 0xffffu) + PV_ADLER - 1u;
    s2 += (adler_a >> 16) + (adler_b >> 16) + PV_ADLER - rem;
    if (s1 >= PV_ADLER) s1 -= PV_ADLER;
    if (s1 >= PV_ADLER) s1 -= PV_ADLER;
    if (s2 >= (PV_ADLER << 1)) s2 -= PV_ADLER << 1;
    if (s2 >= PV_ADLER) s2 -= PV_ADLER;
    return s1 | (s2 << 16);
}

struct PvCrc {                                         // CRC-32 of a PNG chunk's type and data, four bytes per step
    uint32_t c = 0xffffffffu;
    static const uint32_t (*table())[256]
    {
        static const struct Table {
            uint32_t v[4][256];
            Table()
            {
                for (uint32_t i = 0; i < 256; ++i) {
                    uint32_t c = i;
                    for (int b = 0; b < 8; ++b) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
                    v[0][i] = c;
                }
                for (int t = 1; t < 4; ++t)
                    for (uint32_t i = 0; i < 256; ++i) v[t][i] = (v[t - 1][i] >> 8) ^ v[0][v[t - 1][i] & 255u];
            }
        } t;
        return t.v;
    }
    void add(const uint8_t *p, int64_t n)
    {
        const uint32_t (*t)[256] = table();
        int64_t i = 0;
        for (; i + 4 <= n; i += 4) {
            const uint32_t x = c ^ ((uint32_t)p[i] | ((uint32_t)p[i + 1] << 8) | ((uint32_t)p[i + 2] << 16) | ((uint32_t)p[i + 3] << 24));
            c = t[3][x & 255u] ^ t[2][(x >> 8) & 255u] ^ t[1][(x >> 16) & 255u] ^ t[0][x >> 24];
        }
        for (; i < n; ++i) c = t[0][(c ^ p[i]) & 255u] ^ (c >> 8);
    }
};

static inline uint8_t *pv_be32(uint8_t *o, uint32_t v)
{
    o[0] = (uint8_t)(v >> 24); o[1] = (uint8_t)(v >> 16); o[2] = (uint8_t)(v >> 8); o[3] = (uint8_t)v;
    return o + 4;
}
// length, type and data are in place from `chunk` on: appends the CRC
static inline uint8_t *pv_close_chunk(uint8_t *chunk, uint8_t *end)
{
    pv_be32(chunk, (uint32_t)(end - chunk - 8));
    PvCrc crc;
    crc.add(chunk + 4, end - chunk - 4);
    return pv_be32(end, ~crc.c);
}

extern "C" int64_t pca_host_png_assemble(int32_t width, int32_t height, int32_t n_pieces, const void *const *piece, const int64_t *piece_bytes,
                                         uint32_t adler, void *out, int64_t out_cap)
{
    if (width < 1 || height < 1 || n_pieces < 0 || !out || out_cap < 0 || (n_pieces > 0 && (!piece || !piece_bytes))) return -1;
    int64_t body = 2 + 2 + 4;                                      // zlib header, the final block, Adler-32
    for (int k = 0; k < n_pieces; ++k) {
        if (piece_bytes[k] < 0 || (piece_bytes[k] > 0 && !piece[k])) return -1;
        body += piece_bytes[k];
        if (body > INT32_MAX) return -1;                           // a chunk's length is 31 bits
    }
    if (8 + 25 + 12 + body + 12 > out_cap) return -2;
    uint8_t *o = static_cast<uint8_t *>(out);
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    for (int i = 0; i < 8; ++i) *o++ = sig[i];
    uint8_t *chunk = o;
    o += 4;
    *o++ = 'I'; *o++ = 'H'; *o++ = 'D'; *o++ = 'R';
    o = pv_be32(o, (uint32_t)width);
    o = pv_be32(o, (uint32_t)height);
    *o++ = 8; *o++ = 2; *o++ = 0; *o++ = 0; *o++ = 0;              // 8 bits, RGB, deflate, adaptive filtering, no interlace
    o = pv_close_chunk(chunk, o);
    chunk = o;
    o += 4;
    *o++ = 'I'; *o++ = 'D'; *o++ = 'A'; *o++ = 'T';
    *o++ = 0x78; *o++ = 0x01;                                      // deflate, 32 KiB window, fastest
    for (int k = 0; k < n_pieces; ++k) {
        const uint8_t *p = static_cast<const uint8_t *>(piece[k]);
        for (int64_t i = 0; i < piece_bytes[k]; ++i) o[i] = p[i];
        o += piece_bytes[k];
    }
    *o++ = 3; *o++ = 0;                                            // the final block: fixed Huffman, end of block at once
    o = pv_be32(o, adler);
    o = pv_close_chunk(chunk, o);
    chunk = o;
    o += 4;
    *o++ = 'I'; *o++ = 'E'; *o++ = 'N'; *o++ = 'D';
    o = pv_close_chunk(chunk, o);
    return o - static_cast<uint8_t *>(out);
}
