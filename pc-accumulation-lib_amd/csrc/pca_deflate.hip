// pca_deflate.hip -- KZ: the gzip container of a BEV sample made on the device (include/pca.h: pca_deflate_chunks,
// pca_host_crc32_combine, pca_host_gzip_assemble).
//
// The reference writes a sample as gzip(pickle(dict)) on the host (sem_pc_accum.py:280-294).  The planes are fp16 and
// mostly empty cells: runs of equal bytes and of equal half-words.  A chunk of at most 32 KiB of them becomes ONE
// self-contained, byte-aligned piece of a raw DEFLATE stream -- a non-final fixed-Huffman block followed by an empty
// non-final stored block (the sync-flush marker) -- so that pieces concatenate bytewise with stored blocks the host makes.
//   deflate_chunks   one workgroup per chunk, 256 lanes x 128-byte slices.  Tokens are literals and matches at distance 1
//                    or 2; a lane's matches may reach back into the previous lane's slice but never before the chunk's
//                    first byte, and never forward over the end of the slice (a longer run is split there, so a match is
//                    at most 128 long).  Pass 1 counts the lane's bits, a workgroup scan gives bit offsets, pass 2 ORs the
//                    same tokens into an LDS image of the output (ds_or_b32, one per 32 bits), which leaves in 16-byte
//                    stores.  The CRC-32 of the chunk comes from the same LDS copy of the input: slice-by-4 per lane, then
//                    a scan with "multiply by x^(8 * 128 * 2^k) mod P" per level, the partial last slice continued serially.
//   deflate_offsets  one workgroup: exclusive scan of the piece sizes.
//   deflate_compact  one workgroup per chunk: the piece from its slot to its place in the contiguous output.
#include "pca_common.h"

#define DF_BLK 256
#define DF_NW (DF_BLK / PCA_WAVE)
#define DF_SLICE 128                                   // bytes a lane tokenises
#define DF_SLICE_DW (DF_SLICE / 4)
#define DF_CHUNK_MAX (DF_BLK * DF_SLICE)
#define DF_BOUND(n) ((9 * (n) + 7) / 8 + 16)           // literals >= 144 cost 9 bits; header, end of block, marker < 16 bytes
#define DF_SLOT ((DF_BOUND(DF_CHUNK_MAX) + 127) / 128 * 128)
#define DF_POLY 0xedb88320u
static_assert(DF_CHUNK_MAX == PCA_DEFLATE_CHUNK_MAX && DF_SLOT % 128 == 0 && DF_SLOT >= DF_BOUND(DF_CHUNK_MAX) + 16,
              "a slot holds the worst case of a chunk, in whole lines, with a spare 16 bytes for the compaction's reads");
static_assert(sizeof(pca_deflate_chunk) == 16, "the chunk table is read in 8-byte scalar loads");

// ---- GF(2) polynomial arithmetic mod P, reflected (bit 31 = x^0), as zlib's crc32_combine does it
__host__ __device__ constexpr uint32_t df_mulmod(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 31; i >= 0; --i) {
        p ^= b & (0u - ((a >> i) & 1u));
        b = (b >> 1) ^ (DF_POLY & (0u - (b & 1u)));
    }
    return p;
}
__host__ __device__ constexpr uint32_t df_x2n(int n)        // x^(2^n) mod P
{
    uint32_t p = 1u << 30;
    for (int i = 0; i < n; ++i) p = df_mulmod(p, p);
    return p;
}
// x^(8 * DF_SLICE * 2^k) = x^(2^(10 + k)): one constant per level of the scan
#define DF_LEVEL_CONST(k) df_x2n(10 + (k))
static_assert(DF_SLICE == 128, "the level constants assume 2^10 bits per slice; a match is at most 128 long (length codes up to 280)");

// LDS word of dword D of the chunk: slices of 32 dwords, rotated by an XOR so that 32 lanes reading dword j of their own
// slices hit 32 banks
__device__ __forceinline__ int df_swz(int D) { return (D & ~31) | ((D ^ (D >> 5)) & 31); }

// consecutive ones of the 128-bit mask (hi:lo) from bit p on
__device__ __forceinline__ int df_run(uint64_t lo, uint64_t hi, int p)
{
    uint64_t a, b;
    if (p < 64) { a = (lo >> p) | (p ? (hi << (64 - p)) : 0ull); b = hi >> p; }
    else { a = hi >> (p - 64); b = 0; }
    if (~a) return __builtin_ctzll(~a);
    return 64 + (~b ? __builtin_ctzll(~b) : 64);
}

// bit 7 of every byte of x that is zero
__device__ __forceinline__ uint32_t df_zero_bytes(uint32_t x)
{
    return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;
}
// bits 7, 15, 23, 31 -> bits 0..3
__device__ __forceinline__ uint32_t df_nibble(uint32_t m) { return (((m >> 7) * 0x00204081u) >> 21) & 15u; }

struct DfMasks {               // per position of the lane's slice
    uint64_t e1[2];            // byte == the byte before it (never set for the chunk's first byte)
    uint64_t e2[2];            // byte == the byte two before it (never set for the chunk's first two bytes)
    uint64_t ge[2];            // byte >= 144: a 9-bit literal
};

// The lane's tokens, greedily: the longer of the runs at distance 1 and 2 if it is at least 3 long, else a literal.
// EMIT = false counts bits; EMIT = true ORs them into the image from bit `bitpos` on.  Both walk the same masks.
template <bool EMIT>
__device__ __forceinline__ uint32_t df_tokens(const DfMasks &m, int len, const uint32_t *in_w, int slice, uint32_t *img,
                                              uint32_t bitpos)
{
    uint32_t bits = 0;
    uint64_t acc = 0;
    uint32_t accn = bitpos & 31u, wi = bitpos >> 5;
    const uint8_t *in_b = reinterpret_cast<const uint8_t *>(in_w);
    for (int p = 0; p < len;) {
        const int r1 = df_run(m.e1[0], m.e1[1], p), r2 = df_run(m.e2[0], m.e2[1], p);
        int run = r1 >= r2 ? r1 : r2;
        run = run < len - p ? run : len - p;                      // at most DF_SLICE: the codes of lengths 131 .. 258 never occur
        uint32_t tok, nb;
        if (run >= 3) {
            uint32_t lc, eb = 0, ev = 0;
            if (run <= 10) lc = 254u + run;
            else {
                const uint32_t x = run - 3;
                eb = (31u - __builtin_clz(x)) - 2u;
                lc = 261u + 4u * eb + ((x >> eb) & 3u);
                ev = x & ((1u << eb) - 1u);
            }
            const uint32_t hlen = lc < 280u ? 7u : 8u;
            nb = hlen + eb + 5u;
            if (EMIT) {
                const uint32_t h = lc < 280u ? __brev(lc - 256u) >> 25 : __brev(0xc0u + lc - 280u) >> 24;
                const uint32_t dist = r1 >= r2 ? 0u : 16u;          // distance codes 0 and 1, five bits, most significant first
                tok = h | (ev << hlen) | (dist << (hlen + eb));
            }
            p += run;
        } else {
            const uint32_t g = (uint32_t)((p < 64 ? m.ge[0] >> p : m.ge[1] >> (p - 64)) & 1ull);
            nb = 8u + g;
            if (EMIT) {
                const uint32_t v = in_b[4 * (slice * DF_SLICE_DW + ((p >> 2) ^ (slice & 31))) + (p & 3)];
                tok = g ? __brev(0x190u + v - 144u) >> 23 : __brev(0x30u + v) >> 24;
            }
            p += 1;
        }
        bits += nb;
        if (EMIT) {
            acc |= (uint64_t)tok << accn;
            accn += nb;
            if (accn >= 32u) {
                atomicOr(&img[wi++], (uint32_t)acc);
                acc >>= 32;
                accn -= 32u;
            }
        }
    }
    if (EMIT && accn) atomicOr(&img[wi], (uint32_t)acc);
    return bits;
}

__global__ __launch_bounds__(DF_BLK) void deflate_chunks(const uint8_t *__restrict__ src, const pca_deflate_chunk *__restrict__ table,
                                                         uint8_t *__restrict__ slots, uint32_t *__restrict__ sizes,
                                                         uint32_t *__restrict__ crcs)
{
    __shared__ __attribute__((aligned(16))) uint32_t in_w[DF_CHUNK_MAX / 4];
    __shared__ __attribute__((aligned(16))) uint32_t img[DF_SLOT / 4];
    __shared__ uint32_t tab[4][256];
    __shared__ uint32_t st[2][DF_BLK];
    __shared__ uint32_t wsum[DF_NW];

    const int tid = threadIdx.x, c = blockIdx.x;
    const int64_t off = pca_sload(&table[c].offset);
    int n = pca_sload(&table[c].length);
    n = n < 0 ? 0 : (n > DF_CHUNK_MAX ? DF_CHUNK_MAX : n);

    // ---- CRC tables (slice by 4), the zeroed image, the chunk
    uint32_t t0 = (uint32_t)tid;
#pragma unroll
    for (int i = 0; i < 8; ++i) t0 = (t0 >> 1) ^ (DF_POLY & (0u - (t0 & 1u)));
    tab[0][tid] = t0;
    const int img_q = (DF_BOUND(n) + 15) >> 4;                     // 16-byte words the piece can reach
    for (int q = tid; q < img_q; q += DF_BLK) reinterpret_cast<uint4 *>(img)[q] = make_uint4(0, 0, 0, 0);
    {
        const uint8_t *base = src + off;
        const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(base) & 3u);
        // aligned dwords that hold at least one byte of the chunk: none of them can lie on a page the chunk does not touch
        const uint32_t *a = reinterpret_cast<const uint32_t *>(base - sh);
        const int nd = (n + 3) >> 2, K = (int)((sh + (uint32_t)n + 3u) >> 2);
        const int fill = ((n + DF_SLICE - 1) / DF_SLICE) * DF_SLICE_DW;    // whole slices: a lane reads all of its own
        for (int D = tid; D < fill; D += DF_BLK) {
            uint32_t v = 0;
            if (D < nd) {
                const uint32_t lo = pca_ldg(a + D);
                const uint32_t hi = (sh && D + 1 < K) ? pca_ldg(a + D + 1) : 0u;
                v = sh ? (lo >> (8u * sh)) | (hi << (32u - 8u * sh)) : lo;
                if (4 * D + 4 > n) v &= (1u << (8 * (n - 4 * D))) - 1u;
            }
            in_w[df_swz(D)] = v;
        }
    }
    __syncthreads();
    {
        const uint32_t t1 = (t0 >> 8) ^ tab[0][t0 & 255u];
        const uint32_t t2 = (t1 >> 8) ^ tab[0][t1 & 255u];
        const uint32_t t3 = (t2 >> 8) ^ tab[0][t2 & 255u];
        tab[1][tid] = t1; tab[2][tid] = t2; tab[3][tid] = t3;
    }
    __syncthreads();

    // ---- the lane's slice: match masks and, for a whole slice, its CRC state
    const int len = n - tid * DF_SLICE < 0 ? 0 : (n - tid * DF_SLICE > DF_SLICE ? DF_SLICE : n - tid * DF_SLICE);
    DfMasks m = {{0, 0}, {0, 0}, {0, 0}};
    uint32_t crc = 0;
    if (len > 0) {
        const bool whole = len == DF_SLICE;
        crc = tid == 0 ? 0xffffffffu : 0u;                        // the chunk's first slice carries the initial register
        uint32_t pw = tid ? in_w[(tid - 1) * DF_SLICE_DW + (31 ^ ((tid - 1) & 31))] : 0u;
#pragma unroll
        for (int j = 0; j < DF_SLICE_DW; ++j) {
            const uint32_t w = in_w[tid * DF_SLICE_DW + (j ^ (tid & 31))];
            const uint64_t n1 = df_nibble(df_zero_bytes(w ^ ((w << 8) | (pw >> 24))));
            const uint64_t n2 = df_nibble(df_zero_bytes(w ^ ((w << 16) | (pw >> 16))));
            const uint64_t ng = df_nibble((((w & 0x7f7f7f7fu) + 0x70707070u) & w) & 0x80808080u);
            m.e1[j >> 4] |= n1 << (4 * (j & 15));
            m.e2[j >> 4] |= n2 << (4 * (j & 15));
            m.ge[j >> 4] |= ng << (4 * (j & 15));
            if (whole) {
                const uint32_t x = crc ^ w;
                crc = tab[3][x & 255u] ^ tab[2][(x >> 8) & 255u] ^ tab[1][(x >> 16) & 255u] ^ tab[0][x >> 24];
            }
            pw = w;
        }
        if (tid == 0) { m.e1[0] &= ~1ull; m.e2[0] &= ~3ull; }     // nothing before the chunk's first byte is ours to cite
        if (!whole) crc = 0;
    }

    // ---- pass 1: bits per lane, offsets by a scan
    const uint32_t my_bits = df_tokens<false>(m, len, in_w, tid, img, 0);
    const uint32_t incl = wave_incl_scan_add(my_bits);
    if ((tid & 63) == 63) wsum[tid >> 6] = incl;
    st[0][tid] = crc;
    __syncthreads();
    uint32_t before = 3, total = 3;                                // the block header: BFINAL = 0, BTYPE = 01
#pragma unroll
    for (int w = 0; w < DF_NW; ++w) {
        const uint32_t s = wsum[w];
        before += w < (tid >> 6) ? s : 0u;
        total += s;
    }
    // ---- pass 2: the same tokens into the image
    df_tokens<true>(m, len, in_w, tid, img, before + incl - my_bits);
    total += 7 + 3;                                                // end of block (seven zero bits), header of the stored block
    const uint32_t nbytes = ((total + 7) >> 3) + 4;                // ... padded to a byte, LEN = 0000, NLEN = ffff
    if (tid == 0) {
        atomicOr(&img[0], 2u);
        atomicOr(&img[(nbytes - 2) >> 2], 0xffu << (8 * ((nbytes - 2) & 3)));
        atomicOr(&img[(nbytes - 1) >> 2], 0xffu << (8 * ((nbytes - 1) & 3)));
    }

    // ---- CRC: state after slices 0..l, for every l (Hillis-Steele over the lanes, one constant per level)
    int cur = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t ck = k == 0 ? DF_LEVEL_CONST(0) : k == 1 ? DF_LEVEL_CONST(1) : k == 2 ? DF_LEVEL_CONST(2) :
                            k == 3 ? DF_LEVEL_CONST(3) : k == 4 ? DF_LEVEL_CONST(4) : k == 5 ? DF_LEVEL_CONST(5) :
                            k == 6 ? DF_LEVEL_CONST(6) : DF_LEVEL_CONST(7);
        uint32_t v = st[cur][tid];
        if (tid >= (1 << k)) v ^= df_mulmod(st[cur][tid - (1 << k)], ck);
        st[cur ^ 1][tid] = v;
        cur ^= 1;
        __syncthreads();
    }
    const int F = n / DF_SLICE, tail = n % DF_SLICE;               // whole slices, bytes of the partial one
    if (tid == (F < DF_BLK ? F : DF_BLK - 1)) {
        uint32_t s = F == 0 ? 0xffffffffu : st[cur][F - 1];
        const int sl = F < DF_BLK ? F : DF_BLK - 1;                // (tail == 0 when F == DF_BLK)
        for (int j = 0; 4 * j < tail; ++j) {
            const uint32_t w = in_w[sl * DF_SLICE_DW + (j ^ (sl & 31))];
            if (4 * j + 4 <= tail) {
                const uint32_t x = s ^ w;
                s = tab[3][x & 255u] ^ tab[2][(x >> 8) & 255u] ^ tab[1][(x >> 16) & 255u] ^ tab[0][x >> 24];
            } else {
                for (int b = 0; b < tail - 4 * j; ++b) s = tab[0][(s ^ (w >> (8 * b))) & 255u] ^ (s >> 8);
            }
        }
        crcs[c] = ~s;
        sizes[c] = nbytes;
    }

    // ---- the piece, in whole 16-byte words (the image is zero behind its last byte).  The barrier is the one that publishes
    // pass 2's ORs into `img` to the lanes that store it: it does not lean on the CRC scan's barriers above
    __syncthreads();
    uint4 *dst = reinterpret_cast<uint4 *>(slots + (size_t)c * DF_SLOT);
    for (uint32_t q = tid; q < (nbytes + 15u) >> 4; q += DF_BLK) dst[q] = reinterpret_cast<const uint4 *>(img)[q];
}

// offs[i] = sizes[0] + .. + sizes[i - 1], i = 0 .. n (one workgroup)
__global__ __launch_bounds__(DF_BLK) void deflate_offsets(const uint32_t *__restrict__ sizes, int n, uint64_t *__restrict__ offs)
{
    __shared__ uint32_t wsum[DF_NW];
    const int tid = threadIdx.x;
    uint64_t run = 0;
    for (int i0 = 0; i0 < n; i0 += DF_BLK) {
        const int i = i0 + tid;
        const uint32_t v = i < n ? sizes[i] : 0u;
        const uint32_t incl = wave_incl_scan_add(v);
        if ((tid & 63) == 63) wsum[tid >> 6] = incl;
        __syncthreads();
        uint32_t before = 0, tile = 0;
#pragma unroll
        for (int w = 0; w < DF_NW; ++w) {
            const uint32_t s = wsum[w];
            before += w < (tid >> 6) ? s : 0u;
            tile += s;
        }
        if (i < n) offs[i] = run + before + incl - v;
        run += tile;
        __syncthreads();
    }
    if (tid == 0) offs[n] = run;
}

__global__ __launch_bounds__(DF_BLK) void deflate_compact(const uint8_t *__restrict__ slots, const uint32_t *__restrict__ sizes,
                                                          const uint64_t *__restrict__ offs, uint8_t *__restrict__ out)
{
    const int tid = threadIdx.x, c = blockIdx.x;
    const uint32_t size = pca_sload(&sizes[c]);
    uint8_t *dst = out + pca_sload(&offs[c]);
    const uint8_t *slot = slots + (size_t)c * DF_SLOT;
    const uint32_t *slot_w = reinterpret_cast<const uint32_t *>(slot);
    uint32_t head = (uint32_t)((0u - reinterpret_cast<uintptr_t>(dst)) & 3u);      // bytes up to the first aligned dword
    head = head < size ? head : size;
    const uint32_t body = (size - head) >> 2, done = head + 4u * body;
    if ((uint32_t)tid < head) dst[tid] = slot[tid];
    if ((uint32_t)tid < size - done) dst[done + tid] = slot[done + tid];
    uint32_t *dst_w = reinterpret_cast<uint32_t *>(dst + head);
    for (uint32_t k = tid; k < body; k += DF_BLK) {                // slot bytes head + 4k ..: two aligned dwords of the slot
        const uint32_t i = (head + 4u * k) >> 2;
        const uint32_t lo = slot_w[i];
        dst_w[k] = head ? (lo >> (8u * head)) | (slot_w[i + 1] << (32u - 8u * head)) : lo;
    }
}

// internal (pca_host.hip): the side stream of pca_host_d2h_async
int pca_side_begin(pca_ctx *ctx, hipStream_t after);
int pca_side_ticket(pca_ctx *ctx);

static inline int64_t df_offs_bytes(int64_t n_chunks) { return pca_align256(8 * (n_chunks + 1)); }

extern "C" int64_t pca_deflate_workspace_bytes(int64_t n_chunks)
{
    if (n_chunks < 0 || n_chunks > PCA_DEFLATE_MAX_CHUNKS) return -1;
    return 256 + df_offs_bytes(n_chunks) + n_chunks * (int64_t)DF_SLOT;
}

extern "C" int pca_deflate_chunks(pca_ctx *ctx, const void *src, const pca_deflate_chunk *chunk_table, int64_t n_chunks, void *out,
                                  uint32_t *out_sizes, uint32_t *out_crcs, void *workspace, void *stream)
{
    if (!ctx) return -1;
    if (n_chunks < 0 || n_chunks > PCA_DEFLATE_MAX_CHUNKS || (n_chunks > 0 && (!src || !chunk_table || !out || !out_sizes || !out_crcs || !workspace))) {
        ctx->err = "deflate_chunks: bad arguments";
        return -1;
    }
    PCA_CHECK(ctx, hipSetDevice(ctx->device));
    if (pca_side_begin(ctx, (hipStream_t)stream)) return -1;
    hipStream_t s = ctx->d2h_stream;
    if (n_chunks > 0) {
        uint8_t *w = reinterpret_cast<uint8_t *>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
        uint64_t *offs = reinterpret_cast<uint64_t *>(w);
        uint8_t *slots = w + df_offs_bytes(n_chunks);
        hipLaunchKernelGGL(deflate_chunks, dim3((unsigned)n_chunks), dim3(DF_BLK), 0, s, static_cast<const uint8_t *>(src), chunk_table,
                           slots, out_sizes, out_crcs);
        hipLaunchKernelGGL(deflate_offsets, dim3(1), dim3(DF_BLK), 0, s, out_sizes, (int)n_chunks, offs);
        hipLaunchKernelGGL(deflate_compact, dim3((unsigned)n_chunks), dim3(DF_BLK), 0, s, slots, out_sizes, offs, static_cast<uint8_t *>(out));
        PCA_CHECK(ctx, hipGetLastError());
    }
    return pca_side_ticket(ctx);
}

// ---- host: CRC-32 of concatenations, the gzip member
static uint32_t df_x2nmodp(uint64_t n, unsigned k)          // x^(n * 2^k) mod P
{
    static const struct Table { uint32_t v[32]; Table() { for (int i = 0; i < 32; ++i) v[i] = df_x2n(i); } } t;
    uint32_t p = 1u << 31;
    for (; n; n >>= 1, ++k)
        if (n & 1) p = df_mulmod(t.v[k & 31], p);
    return p;
}

extern "C" uint32_t pca_host_crc32_combine(uint32_t crc_a, uint32_t crc_b, int64_t len_b)
{
    if (len_b <= 0) return len_b == 0 ? crc_a : 0;
    return df_mulmod(df_x2nmodp((uint64_t)len_b, 3), crc_a) ^ crc_b;
}

static uint32_t df_host_crc32(const uint8_t *p, int64_t n)
{
    static const struct Table {
        uint32_t v[256];
        Table() { for (uint32_t i = 0; i < 256; ++i) { uint32_t c = i; for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (DF_POLY & (0u - (c & 1u))); v[i] = c; } }
    } t;
    uint32_t c = 0xffffffffu;
    for (int64_t i = 0; i < n; ++i) c = t.v[(c ^ p[i]) & 255u] ^ (c >> 8);
    return ~c;
}

extern "C" int64_t pca_host_gzip_assemble(int32_t n_pieces, const void *const *piece, const int64_t *piece_bytes, const int64_t *raw_bytes,
                                          const uint32_t *crc, void *out, int64_t out_cap)
{
    if (n_pieces < 0 || !out || out_cap < 0 || (n_pieces > 0 && (!piece || !piece_bytes || !raw_bytes || !crc))) return -1;
    int64_t need = 10 + 2 + 8;
    for (int k = 0; k < n_pieces; ++k) {
        if (piece_bytes[k] < 0 || (piece_bytes[k] > 0 && !piece[k])) return -1;
        need += piece_bytes[k] + (raw_bytes[k] < 0 ? 5 * ((piece_bytes[k] + 65534) / 65535) : 0);
    }
    if (need > out_cap) return -2;
    uint8_t *o = static_cast<uint8_t *>(out);
    const uint8_t header[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 255};       // deflate, no flags, no time, unknown system
    for (int i = 0; i < 10; ++i) *o++ = header[i];
    uint32_t total_crc = 0;
    uint64_t total_len = 0;
    for (int k = 0; k < n_pieces; ++k) {
        const uint8_t *p = static_cast<const uint8_t *>(piece[k]);
        const int64_t nb = piece_bytes[k];
        if (raw_bytes[k] >= 0) {                                   // a byte-aligned piece of a deflate stream: as it is
            for (int64_t i = 0; i < nb; ++i) o[i] = p[i];
            o += nb;
            total_crc = pca_host_crc32_combine(total_crc, crc[k], raw_bytes[k]);
            total_len += (uint64_t)raw_bytes[k];
            continue;
        }
        for (int64_t at = 0; at < nb; at += 65535) {               // raw bytes: non-final stored blocks
            const int64_t l = nb - at < 65535 ? nb - at : 65535;
            *o++ = 0;
            *o++ = (uint8_t)(l & 255); *o++ = (uint8_t)(l >> 8);
            *o++ = (uint8_t)(~l & 255); *o++ = (uint8_t)((~l >> 8) & 255);
            for (int64_t i = 0; i < l; ++i) o[i] = p[at + i];
            o += l;
        }
        total_crc = pca_host_crc32_combine(total_crc, df_host_crc32(p, nb), nb);
        total_len += (uint64_t)nb;
    }
    *o++ = 3; *o++ = 0;                                            // the final block: fixed Huffman, end of block at once
    for (int i = 0; i < 4; ++i) *o++ = (uint8_t)(total_crc >> (8 * i));
    for (int i = 0; i < 4; ++i) *o++ = (uint8_t)(total_len >> (8 * i));
    return o - static_cast<uint8_t *>(out);
}
