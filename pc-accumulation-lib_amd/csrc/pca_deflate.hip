// pca_deflate.hip -- KZ: the gzip container of a BEV sample made on the device (include/pca.h: pca_deflate_chunks,
// pca_deflate_chunks_dyn, pca_host_crc32_combine, pca_host_gzip_assemble).
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
//   deflate_chunks_dyn  the same chunk, tokens and piece, with the entropy coder chosen per chunk: fixed as above, or a
//                    Huffman code of the chunk's own (BTYPE 10) built in the workgroup, whichever takes fewer bits.
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

// ---- coders: what a token costs and how it is written.  A token is a literal v (g: v >= 144) or a match of length code lc
// with eb extra bits of value ev at distance 1 (d2 = false) or 2.  count() sees every token of a counting walk.
#define DF_NSYM 288                                    // literal/length symbols a table holds (286 .. 287 never occur)
#define DF_EOB 256
struct DfFixed {                                       // BTYPE 01
    static constexpr bool READS_LITERAL = false;       // a counting walk needs g alone
    __device__ __forceinline__ uint32_t lit_bits(uint32_t, uint32_t g) const { return 8u + g; }
    __device__ __forceinline__ uint32_t lit_code(uint32_t v, uint32_t g) const
    {
        return g ? __brev(0x190u + v - 144u) >> 23 : __brev(0x30u + v) >> 24;
    }
    __device__ __forceinline__ uint32_t match_bits(uint32_t lc, uint32_t eb) const { return (lc < 280u ? 7u : 8u) + eb + 5u; }
    __device__ __forceinline__ uint32_t match_code(uint32_t lc, uint32_t eb, uint32_t ev, bool d2) const
    {
        const uint32_t hlen = lc < 280u ? 7u : 8u;
        const uint32_t h = lc < 280u ? __brev(lc - 256u) >> 25 : __brev(0xc0u + lc - 280u) >> 24;
        const uint32_t dist = d2 ? 16u : 0u;                    // distance codes 0 and 1, five bits, most significant first
        return h | (ev << hlen) | (dist << (hlen + eb));
    }
    __device__ __forceinline__ void count(uint32_t) const {}
};
struct DfFixedHist : DfFixed {                         // the fixed cost, and the histogram a dynamic code is built from
    static constexpr bool READS_LITERAL = true;
    uint32_t *hist;                                    // LDS, DF_NSYM counters
    __device__ __forceinline__ void count(uint32_t sym) const { atomicAdd(&hist[sym], 1u); }
};
struct DfDyn {                                         // BTYPE 10: codes[s] = the code of s, bit-reversed, | its length << 16
    static constexpr bool READS_LITERAL = true;
    const uint32_t *codes;                             // LDS, DF_NSYM entries; both distance codes are one bit long
    __device__ __forceinline__ uint32_t lit_bits(uint32_t v, uint32_t) const { return codes[v] >> 16; }
    __device__ __forceinline__ uint32_t lit_code(uint32_t v, uint32_t) const { return codes[v] & 0xffffu; }
    __device__ __forceinline__ uint32_t match_bits(uint32_t lc, uint32_t eb) const { return (codes[lc] >> 16) + eb + 1u; }
    __device__ __forceinline__ uint32_t match_code(uint32_t lc, uint32_t eb, uint32_t ev, bool d2) const
    {
        const uint32_t e = codes[lc], hlen = e >> 16;
        return (e & 0xffffu) | (ev << hlen) | ((d2 ? 1u : 0u) << (hlen + eb));
    }
    __device__ __forceinline__ void count(uint32_t) const {}
};

// How a lane's slice falls into tokens, as a walk that has found it leaves it for the walks that follow: they then need
// neither match mask.  A literal is one byte, a match at least three, so the starts alone give the lengths.
struct DfSplit {
    uint64_t start[2];         // a token starts at this position
    uint64_t d2[2];            // ... and it is a match at distance 2
};
enum { DF_WALK_SCAN, DF_WALK_RECORD, DF_WALK_REPLAY };  // find the tokens / find them and fill `sp` in / take them from `sp`

// The lane's tokens, greedily: the longer of the runs at distance 1 and 2 if it is at least 3 long, else a literal.
// EMIT = false counts bits; EMIT = true ORs them into the image from bit `bitpos` on.  Both walk the same masks (or the
// split a walk made of them), whatever the coder: a token is at most 15 + 5 + 1 bits long.
template <bool EMIT, class CODER, int WALK = DF_WALK_SCAN>
__device__ __forceinline__ uint32_t df_tokens(const CODER &cd, const DfMasks &m, int len, const uint32_t *in_w, int slice,
                                              uint32_t *img, uint32_t bitpos, DfSplit *sp = nullptr)
{
    uint32_t bits = 0;
    uint64_t acc = 0;
    uint32_t accn = bitpos & 31u, wi = bitpos >> 5;
    const uint8_t *in_b = reinterpret_cast<const uint8_t *>(in_w);
    uint64_t s0 = 0, s1 = 0, t0 = 0, t1 = 0;                       // the split: starts (to come, when replayed), distance-2 flags
    if (WALK == DF_WALK_REPLAY) { s0 = sp->start[0]; s1 = sp->start[1]; t0 = sp->d2[0]; t1 = sp->d2[1]; }
    for (int p = 0; p < len;) {
        int run;
        bool d2;
        if (WALK != DF_WALK_REPLAY) {
            const int r1 = df_run(m.e1[0], m.e1[1], p), r2 = df_run(m.e2[0], m.e2[1], p);
            run = r1 >= r2 ? r1 : r2;
            run = run < len - p ? run : len - p;                  // at most DF_SLICE: the codes of lengths 131 .. 258 never occur
            d2 = r1 < r2;
            if (WALK == DF_WALK_RECORD) {
                const uint64_t bit = 1ull << (p & 63);
                if (p < 64) { s0 |= bit; t0 |= run >= 3 && d2 ? bit : 0ull; }
                else { s1 |= bit; t1 |= run >= 3 && d2 ? bit : 0ull; }
            }
        } else {                                                  // p is the lowest start left: up to the next one, or the end
            if (p < 64) s0 &= s0 - 1ull;
            else s1 &= s1 - 1ull;
            const int next = s0 ? __builtin_ctzll(s0) : (s1 ? 64 + __builtin_ctzll(s1) : len);
            run = next - p;
            d2 = ((p < 64 ? t0 >> p : t1 >> (p - 64)) & 1ull) != 0;
        }
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
            nb = cd.match_bits(lc, eb);
            if (EMIT) tok = cd.match_code(lc, eb, ev, d2);
            else cd.count(lc);
            p += run;
        } else {
            const uint32_t g = (uint32_t)((p < 64 ? m.ge[0] >> p : m.ge[1] >> (p - 64)) & 1ull);
            uint32_t v = 0;
            if (EMIT || CODER::READS_LITERAL) v = in_b[4 * (slice * DF_SLICE_DW + ((p >> 2) ^ (slice & 31))) + (p & 3)];
            nb = cd.lit_bits(v, g);
            if (EMIT) tok = cd.lit_code(v, g);
            else cd.count(v);
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
    if (WALK == DF_WALK_RECORD) { sp->start[0] = s0; sp->start[1] = s1; sp->d2[0] = t0; sp->d2[1] = t1; }
    return bits;
}

// ---- what the two chunk kernels share around the coder
// CRC tables (slice by 4), the zeroed image, the chunk in LDS.  Returns the chunk's length, behind a barrier.
__device__ __forceinline__ int df_stage(const uint8_t *__restrict__ src, const pca_deflate_chunk *__restrict__ table, int c,
                                        uint32_t *in_w, uint32_t *img, uint32_t (*tab)[256])
{
    const int tid = threadIdx.x;
    const int64_t off = pca_sload(&table[c].offset);
    int n = pca_sload(&table[c].length);
    n = n < 0 ? 0 : (n > DF_CHUNK_MAX ? DF_CHUNK_MAX : n);
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
    return n;
}

// the lane's slice: its length, match masks and, for a whole slice, its CRC state
__device__ __forceinline__ int df_slice(const uint32_t *in_w, const uint32_t (*tab)[256], int n, DfMasks &m, uint32_t &crc)
{
    const int tid = threadIdx.x;
    const int len = n - tid * DF_SLICE < 0 ? 0 : (n - tid * DF_SLICE > DF_SLICE ? DF_SLICE : n - tid * DF_SLICE);
    m = {{0, 0}, {0, 0}, {0, 0}};
    crc = 0;
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
    return len;
}

// CRC of the chunk from the lanes' slice states: state after slices 0..l, for every l (Hillis-Steele over the lanes, one
// constant per level), the partial last slice continued serially by one lane, which writes the word.  Every barrier in
// here is passed by all lanes; `st` is free again behind the next barrier of the caller.
__device__ __forceinline__ void df_crc(uint32_t (*st)[DF_BLK], const uint32_t (*tab)[256], const uint32_t *in_w, int n,
                                       uint32_t crc, uint32_t *crc_out)
{
    const int tid = threadIdx.x;
    st[0][tid] = crc;
    __syncthreads();
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
        *crc_out = ~s;
    }
}

// sum over the workgroup of the lanes' bit counts: (bits of the lanes before this one, bits of all).  One barrier.
__device__ __forceinline__ void df_bit_offsets(uint32_t my_bits, uint32_t *wsum, uint32_t &before, uint32_t &total)
{
    const int tid = threadIdx.x;
    const uint32_t incl = wave_incl_scan_add(my_bits);
    if ((tid & 63) == 63) wsum[tid >> 6] = incl;
    __syncthreads();
    before = incl - my_bits;
    total = 0;
#pragma unroll
    for (int w = 0; w < DF_NW; ++w) {
        const uint32_t s = wsum[w];
        before += w < (tid >> 6) ? s : 0u;
        total += s;
    }
}

// the end of a piece whose blocks take `total` bits: the header of the empty stored block, padding to a byte, LEN = 0000,
// NLEN = ffff (one lane).  Returns the piece's bytes.
__device__ __forceinline__ uint32_t df_marker(uint32_t *img, uint32_t total)
{
    const uint32_t nbytes = ((total + 3 + 7) >> 3) + 4;
    if (threadIdx.x == 0) {
        atomicOr(&img[(nbytes - 2) >> 2], 0xffu << (8 * ((nbytes - 2) & 3)));
        atomicOr(&img[(nbytes - 1) >> 2], 0xffu << (8 * ((nbytes - 1) & 3)));
    }
    return nbytes;
}

// the piece, in whole 16-byte words (the image is zero behind its last byte).  The barrier is the one that publishes the
// ORs into `img` to the lanes that store it
__device__ __forceinline__ void df_store(const uint32_t *img, uint32_t nbytes, uint8_t *__restrict__ slots, int c)
{
    __syncthreads();
    uint4 *dst = reinterpret_cast<uint4 *>(slots + (size_t)c * DF_SLOT);
    for (uint32_t q = threadIdx.x; q < (nbytes + 15u) >> 4; q += DF_BLK) dst[q] = reinterpret_cast<const uint4 *>(img)[q];
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
    const int n = df_stage(src, table, c, in_w, img, tab);
    DfMasks m;
    uint32_t crc;
    const int len = df_slice(in_w, tab, n, m, crc);

    // ---- pass 1: bits per lane, offsets by a scan; pass 2: the same tokens into the image
    const DfFixed cd{};
    const uint32_t my_bits = df_tokens<false>(cd, m, len, in_w, tid, img, 0);
    uint32_t before, total;
    df_bit_offsets(my_bits, wsum, before, total);
    df_tokens<true>(cd, m, len, in_w, tid, img, 3 + before);      // behind the block header: BFINAL = 0, BTYPE = 01
    if (tid == 0) atomicOr(&img[0], 2u);
    const uint32_t nbytes = df_marker(img, 3 + total + 7);         // end of block: seven zero bits
    if (tid == 0) sizes[c] = nbytes;
    df_crc(st, tab, in_w, n, crc, &crcs[c]);
    df_store(img, nbytes, slots, c);
}

// ---- the dynamic coder's tables, built per workgroup from the histogram of pass 1
#define DF_SORT 512                                    // keys of the bitonic sort: two per lane
#define DF_MAXBITS 15
#define DF_KEY_NONE 0xffffffffu                        // an unused symbol: sorts behind every used one
#define DF_W_NONE 0xffffffffu                          // weight of a tree node that does not exist (yet)
#define DF_HDR_DW 64                                   // 17 + 57 + at most 6 bits per code length of 288 < 2048 bits
static_assert(DF_SORT == 2 * DF_BLK && DF_NSYM <= DF_SORT && DF_NSYM - DF_BLK <= DF_BLK, "two keys, two symbols per lane");

// The code-length alphabet is ONE fixed complete code (lengths <= 7, so every HCLEN entry fits its three bits):
// three bits for 0 and the zero runs 17 and 18, four for the lengths 4 .. 10 and the repeat 16, six for the rest.
struct DfClCode {
    uint32_t code[19];                                 // bit-reversed code | length << 16, by symbol
    uint64_t hclen;                                    // the 19 three-bit lengths in the order the format sends them
};
__host__ __device__ constexpr DfClCode df_make_cl_code()
{
    constexpr int len[19] = {3, 6, 6, 6, 4, 4, 4, 4, 4, 4, 4, 6, 6, 6, 6, 6, 4, 3, 3};
    constexpr int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    DfClCode t = {};
    uint32_t next = 0;
    for (int l = 1; l <= 7; ++l) {
        for (int s = 0; s < 19; ++s) {
            if (len[s] != l) continue;
            uint32_t r = 0;
            for (int b = 0; b < l; ++b) r |= ((next >> b) & 1u) << (l - 1 - b);
            t.code[s] = r | ((uint32_t)l << 16);
            ++next;
        }
        next <<= 1;
    }
    for (int i = 0; i < 19; ++i) t.hclen |= (uint64_t)len[order[i]] << (3 * i);
    return t;
}
constexpr bool df_cl_complete()
{
    constexpr int len[19] = {3, 6, 6, 6, 4, 4, 4, 4, 4, 4, 4, 6, 6, 6, 6, 6, 4, 3, 3};
    int kraft = 0;
    for (int s = 0; s < 19; ++s) kraft += 128 >> len[s];
    return kraft == 128 && df_make_cl_code().code[15] == (63u | (6u << 16));
}
static_assert(df_cl_complete(), "the code-length code must be complete: inflate rejects any other");
// The table as immediates -- seven symbols of (length << 6 | code) per 64-bit word -- so that a lane looks a symbol up with
// shifts, not with a load per code length.
__host__ __device__ constexpr uint64_t df_cl_pack(int k)
{
    const DfClCode t = df_make_cl_code();
    uint64_t w = 0;
    for (int i = 0; i < 7 && 7 * k + i < 19; ++i)
        w |= (uint64_t)((t.code[7 * k + i] & 63u) | ((t.code[7 * k + i] >> 16) << 6)) << (9 * i);
    return w;
}

struct DfBitCounter {                                  // the counting walk of a header run
    uint32_t bits;
    __device__ __forceinline__ void put(uint32_t, uint32_t nb) { bits += nb; }
};
struct DfOrWriter {                                    // bits ORed into zeroed LDS words from any bit position on
    uint32_t *w;
    uint64_t acc;
    uint32_t accn, wi;
    __device__ __forceinline__ DfOrWriter(uint32_t *words, uint32_t bitpos) : w(words), acc(0), accn(bitpos & 31u), wi(bitpos >> 5) {}
    __device__ __forceinline__ void put(uint32_t v, uint32_t nb)
    {
        acc |= (uint64_t)v << accn;
        accn += nb;
        if (accn >= 32u) {
            atomicOr(&w[wi++], (uint32_t)acc);
            acc >>= 32;
            accn -= 32u;
        }
    }
    __device__ __forceinline__ void flush() { if (accn) atomicOr(&w[wi], (uint32_t)acc); }
};
template <class W>
__device__ __forceinline__ void df_put_cl(W &bw, uint32_t sym)
{
    constexpr uint64_t p0 = df_cl_pack(0), p1 = df_cl_pack(1), p2 = df_cl_pack(2);
    const uint64_t w = sym < 7u ? p0 : (sym < 14u ? p1 : p2);
    const uint32_t e = (uint32_t)(w >> (9u * (sym < 7u ? sym : (sym < 14u ? sym - 7u : sym - 14u)))) & 511u;
    bw.put(e & 63u, e >> 6);
}

// One run of `r` equal code lengths `v`, as zlib's send_tree cuts it: zeros in runs of 11 .. 138 (18) and 3 .. 10 (17),
// other lengths once and then in repeats of 3 .. 6 (16).  At most 6 bits per length.  r <= DF_NSYM bounds every loop.
template <class W>
__device__ __forceinline__ void df_put_run(W &bw, uint32_t v, uint32_t r)
{
    if (v == 0) {
        for (int i = 0; i < DF_NSYM / 11 + 1 && r >= 11u; ++i) {
            const uint32_t t = r < 138u ? r : 138u;
            df_put_cl(bw, 18);
            bw.put(t - 11u, 7);
            r -= t;
        }
        if (r >= 3u) {
            df_put_cl(bw, 17);
            bw.put(r - 3u, 3);
            r = 0;
        }
    } else {
        df_put_cl(bw, v);
        --r;
        for (int i = 0; i < DF_NSYM / 3 + 1 && r >= 3u; ++i) {
            const uint32_t t = r < 6u ? r : 6u;
            df_put_cl(bw, 16);
            bw.put(t - 3u, 2);
            r -= t;
        }
    }
    for (int i = 0; i < 2 && r > 0u; ++i, --r) df_put_cl(bw, v);   // what is left is shorter than any run symbol takes
}

#define DF_HDR_FIXED (17 + 3 * 19)                     // bits of a header before the code lengths
#define DF_RUN_DW ((DF_NSYM + 32) / 32)                // one bit per code length, one behind the last: where a run starts

// words of the workgroup's small state
enum { DF_S_NUSED, DF_S_MAXSYM, DF_S_HBITS, DF_S_WORDS };

// deflate_chunks_dyn: per chunk the smaller of the fixed-Huffman piece deflate_chunks makes and a dynamic-Huffman piece
// (BTYPE 10) of the same tokens, by exact bit count, a tie to fixed.
//   pass 1 counts the fixed bits and, with ds_add, the literal/length symbols (end of block counts 1), and keeps where
//   the lane's tokens start, so that the walks after it do not search the match masks again;
//   the used symbols are sorted by count (bitonic, 512 keys), one lane merges them into a Huffman tree with two queues
//   (ties to the leaf: the shallowest of the optimal trees), every leaf walks up to the root for its depth, depths above
//   15 are cut and the Kraft sum repaired one unit per step (at most one step per symbol), lengths go back to the
//   symbols by rank, canonical codes come from counts per length and a prefix sum, bit-reversed;
//   the header sends HLIT up to the highest used symbol, two distance codes of one bit each whatever the chunk holds
//   (a complete code), and the code lengths through the fixed code-length code above, with its run symbols: a lane per
//   run of equal lengths, placed by a scan like the tokens are;
//   a second count with the new lengths lays the dynamic piece out; then pass 2 with them behind the header, or today's.
// Every loop of the build has a constant bound on its trip count.
__global__ __launch_bounds__(DF_BLK) void deflate_chunks_dyn(const uint8_t *__restrict__ src, const pca_deflate_chunk *__restrict__ table,
                                                             uint8_t *__restrict__ slots, uint32_t *__restrict__ sizes,
                                                             uint32_t *__restrict__ crcs)
{
    __shared__ __attribute__((aligned(16))) uint32_t in_w[DF_CHUNK_MAX / 4];
    __shared__ __attribute__((aligned(16))) uint32_t img[DF_SLOT / 4];
    __shared__ uint32_t tab[4][256];
    __shared__ uint32_t st[2][DF_BLK];                 // the CRC scan, then the sort keys
    __shared__ uint32_t wsum[DF_NW];
    __shared__ uint32_t hist[DF_NSYM];                 // symbol counts, then the weights of the tree's inner nodes
    __shared__ uint32_t codes[DF_NSYM];                // DfDyn
    __shared__ uint16_t parent[2][DF_NSYM];            // of leaf i (by rank) / of inner node j: an inner node
    __shared__ __attribute__((aligned(4))) uint8_t lens[DF_NSYM];
    __shared__ uint32_t hdr[DF_HDR_DW], run_start[DF_RUN_DW];
    __shared__ uint32_t blc[DF_MAXBITS + 1], next_code[DF_MAXBITS + 1], len_count[DF_NW + 1][DF_MAXBITS + 1];
    __shared__ uint32_t state[DF_S_WORDS];
    static_assert(sizeof(in_w) + sizeof(img) + sizeof(tab) + sizeof(st) + sizeof(wsum) + sizeof(hist) + sizeof(codes) +
                  sizeof(parent) + sizeof(lens) + sizeof(hdr) + sizeof(run_start) + sizeof(blc) + sizeof(next_code) + sizeof(len_count) + sizeof(state) <= 80 * 1024,
                  "two workgroups per CU: half of the 160 KiB each");
    static_assert(sizeof(st) == DF_SORT * sizeof(uint32_t), "the keys take the CRC scan's place");
    uint32_t *keys = &st[0][0], *node_w = hist;

    const int tid = threadIdx.x, c = blockIdx.x;
    for (int s = tid; s < DF_NSYM; s += DF_BLK) { hist[s] = 0; lens[s] = 0; }
    if (tid <= DF_MAXBITS) blc[tid] = 0;
    if (tid < DF_S_WORDS) state[tid] = 0;
    if (tid < DF_HDR_DW) hdr[tid] = 0;
    if (tid < DF_RUN_DW) run_start[tid] = 0;
    const int n = df_stage(src, table, c, in_w, img, tab);         // (its barriers publish the zeros above)
    DfMasks m;
    uint32_t crc;
    const int len = df_slice(in_w, tab, n, m, crc);
    df_crc(st, tab, in_w, n, crc, &crcs[c]);

    // ---- pass 1: fixed bits per lane and the histogram
    DfFixedHist cf;
    cf.hist = hist;
    DfSplit sp;
    const uint32_t fixed_bits = df_tokens<false, DfFixedHist, DF_WALK_RECORD>(cf, m, len, in_w, tid, img, 0, &sp);
    if (tid == 0) atomicAdd(&hist[DF_EOB], 1u);
    uint32_t fixed_before, fixed_total;
    df_bit_offsets(fixed_bits, wsum, fixed_before, fixed_total);  // (its barrier: the histogram is whole, `st` is free)
    fixed_total += 3 + 7;

    // ---- used symbols by ascending count: key = count << 9 | symbol (a count is at most 32769)
    for (int i = tid; i < DF_SORT; i += DF_BLK) {
        const uint32_t cnt = i < 286 ? hist[i] : 0u;
        keys[i] = cnt ? (cnt << 9) | (uint32_t)i : DF_KEY_NONE;
    }
    __syncthreads();
    for (int k = 2; k <= DF_SORT; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int i = ((tid & ~(j - 1)) << 1) | (tid & (j - 1)), p = i | j;
            const uint32_t a = keys[i], b = keys[p];
            if ((a > b) == ((i & k) == 0)) { keys[i] = b; keys[p] = a; }
            __syncthreads();
        }
    }
    for (int i = tid; i < DF_SORT; i += DF_BLK) {
        if (keys[i] != DF_KEY_NONE && (i == DF_SORT - 1 || keys[i + 1] == DF_KEY_NONE)) state[DF_S_NUSED] = (uint32_t)i + 1u;
        if (i < DF_NSYM) node_w[i] = DF_W_NONE;                     // the histogram is in the keys now
    }
    __syncthreads();
    const int nu = (int)state[DF_S_NUSED];                         // 1 .. 286: end of block is always there

    // ---- the tree: inner node k joins the two lightest of the leaves and nodes not joined yet
    // (a leaf behind the last reads as 2^23 - 1, a node not made yet as DF_W_NONE: both above any weight there is, and
    // while a node is to be made two real items are left; no branches: this is one lane's chain of LDS round trips)
    if (tid == 0 && nu >= 2) {
        uint16_t *par = &parent[0][0];
        uint32_t li = 0, ni = 0;
        for (int k = 0; k < DF_NSYM && k < nu - 1; ++k) {
            const uint32_t l0 = keys[li] >> 9, l1 = keys[li + 1] >> 9;
            const uint32_t n0 = node_w[ni], n1 = node_w[ni + 1];   // ni + 1 <= k + 1 < DF_NSYM
            const bool f = l0 <= n0;                               // the lighter one: a leaf? (ties to the leaf)
            const uint32_t x = f ? l1 : l0, y = f ? n0 : n1;       // the heads behind it
            const bool g = x <= y;
            par[f ? li : DF_NSYM + ni] = (uint16_t)k;
            li += f ? 1u : 0u; ni += f ? 0u : 1u;
            par[g ? li : DF_NSYM + ni] = (uint16_t)k;
            li += g ? 1u : 0u; ni += g ? 0u : 1u;
            node_w[k] = (f ? l0 : n0) + (g ? x : y);
        }
    }
    if (tid == 0 && nu < 2) {           // end of block alone: an unused symbol gets the other one-bit code
        lens[DF_EOB] = 1; lens[0] = 1;
        blc[1] = 2;
        state[DF_S_MAXSYM] = DF_EOB;
    }
    __syncthreads();

    // ---- depth of every leaf (the root is node nu - 2), counted per length with everything deeper than 15 at 15
    if (nu >= 2) {
        for (int i = tid; i < nu; i += DF_BLK) {
            uint32_t d = 1, p = parent[0][i];
            for (int t = 0; t < DF_NSYM && p != (uint32_t)(nu - 2); ++t) { p = parent[1][p]; ++d; }
            atomicAdd(&blc[d < DF_MAXBITS ? d : DF_MAXBITS], 1u);
        }
    }
    __syncthreads();
    // ---- Kraft repair: in units of 2^-15 the cut leaves weigh 1 each instead of less, so the sum exceeds 2^15 by fewer
    // units than there are symbols.  A step takes one unit off: a leaf leaves length 15, and the longest code shorter than
    // 15 moves one level down with it (one code of length l becomes two of l + 1: the sum keeps its value).
    if (tid == 0) {
        uint32_t total = 0;
        for (int l = 1; l <= DF_MAXBITS; ++l) total += blc[l] << (DF_MAXBITS - l);
        for (int it = 0; it < DF_NSYM && total > (1u << DF_MAXBITS); ++it) {
            blc[DF_MAXBITS] -= 1;
            for (int l = DF_MAXBITS - 1; l > 0; --l)
                if (blc[l]) { blc[l] -= 1; blc[l + 1] += 2; break; }
            --total;
        }
        uint32_t code = 0;
        for (int l = 1; l <= DF_MAXBITS; ++l) {
            code = (code + (l > 1 ? blc[l - 1] : 0u)) << 1;
            next_code[l] = code;
        }
    }
    __syncthreads();
    // ---- lengths by rank: the rarest symbols take the longest codes.  Where nothing was cut these are the tree's depths
    // up to a swap among equal counts, so the cost is the optimum
    if (nu >= 2) {
        for (int i = tid; i < nu; i += DF_BLK) {
            const uint32_t sym = keys[i] & 511u;
            uint32_t l = 0, cum = 0;
            for (int b = DF_MAXBITS; b > 0; --b) {
                cum += blc[b];
                if (l == 0 && (uint32_t)i < cum) l = (uint32_t)b;
            }
            lens[sym] = (uint8_t)l;
            atomicMax(&state[DF_S_MAXSYM], sym);
        }
    }
    __syncthreads();
    const int n_ll = (int)state[DF_S_MAXSYM] + 1;                  // HLIT: 257 .. 286 codes

    // ---- canonical codes: symbol order within a length.  Symbols sit on lanes in order (0 .. 255, then 256 .. on the first
    // lanes), so a ballot per length ranks a symbol within its wave and counts the wave's; the waves before add up
    uint32_t sym_l[2], sym_rank[2] = {0, 0};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int s = tid + k * DF_BLK;
        const uint32_t l = s < DF_NSYM ? lens[s] : 0u;
        sym_l[k] = l;
        for (uint32_t b = 1; b <= DF_MAXBITS; ++b) {
            const uint64_t same = __ballot(l == b);
            if (l == b) sym_rank[k] = (uint32_t)__builtin_popcountll(same & ((1ull << (tid & 63)) - 1ull));
            if ((tid & 63) == 0 && (k == 0 || tid == 0)) len_count[k ? DF_NW : tid >> 6][b] = (uint32_t)__builtin_popcountll(same);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const uint32_t l = sym_l[k];
        if (l) {
            uint32_t rank = sym_rank[k];
            for (int g = 0; g < (k ? DF_NW : tid >> 6); ++g) rank += len_count[g][l];
            codes[tid + k * DF_BLK] = (__brev(next_code[l] + rank) >> (32u - l)) | (l << 16);
        }
    }
    // ---- the header: where a run of equal code lengths starts (the n_ll lengths, then the two distance lengths), ...
    const int n_cl = n_ll + 2;
    uint32_t my_v[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int p = tid + k * DF_BLK;
        const uint32_t v = p < n_ll ? lens[p] : 1u, u = p - 1 < n_ll ? lens[p > 0 ? p - 1 : 0] : 1u;
        my_v[k] = v;
        if (p <= n_cl && (p == 0 || p == n_cl || v != u)) atomicOr(&run_start[p >> 5], 1u << (p & 31));
    }
    __syncthreads();
    // ... how long the run of a lane that starts one is, what it costs, where its bits go, and the bits
    uint32_t my_r[2], my_b[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int p = tid + k * DF_BLK;
        my_r[k] = 0;
        if (p < n_cl && ((run_start[p >> 5] >> (p & 31)) & 1u)) {
            int q = DF_NSYM;                                       // the next start: there is one at n_cl
            uint32_t w = run_start[p >> 5] & ((0xfffffffeu << (p & 31)));
            for (int d = p >> 5; d < DF_RUN_DW; ++d) {
                if (d > (p >> 5)) w = run_start[d];
                if (w) { q = 32 * d + __builtin_ctz(w); break; }
            }
            my_r[k] = (uint32_t)(q - p);
        }
        DfBitCounter bc = {0};
        if (my_r[k]) df_put_run(bc, my_v[k], my_r[k]);
        my_b[k] = bc.bits;
    }
    uint32_t hdr_before, hdr_first;
    df_bit_offsets(my_b[0], wsum, hdr_before, hdr_first);          // positions 0 .. 255, then 256 .. in the first lanes
    const uint32_t incl2 = wave_incl_scan_add(my_b[1]);
    if (tid == PCA_WAVE - 1) state[DF_S_HBITS] = DF_HDR_FIXED + hdr_first + incl2;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (my_r[k]) {
            DfOrWriter bw(hdr, DF_HDR_FIXED + (k == 0 ? hdr_before : hdr_first + incl2 - my_b[1]));
            df_put_run(bw, my_v[k], my_r[k]);
            bw.flush();
        }
    }
    if (tid == 0) {
        constexpr uint64_t hclen = df_make_cl_code().hclen;
        DfOrWriter bw(hdr, 0);
        bw.put(4u | ((uint32_t)(n_ll - 257) << 3) | (1u << 8) | (15u << 13), 17);   // BFINAL 0, BTYPE 10, HLIT, HDIST 1, HCLEN 15
        bw.put((uint32_t)(hclen & 0x3fffffffu), 30);
        bw.put((uint32_t)(hclen >> 30), 27);
        bw.flush();
    }
    __syncthreads();

    // ---- the choice, by exact bit count (both pieces end in the same marker): the dynamic piece is laid out first, so
    // what is compared is what would be written
    DfDyn cd;
    cd.codes = codes;
    const uint32_t hbits = state[DF_S_HBITS], eob = codes[DF_EOB];
    const uint32_t my_bits = df_tokens<false, DfDyn, DF_WALK_REPLAY>(cd, m, len, in_w, tid, img, 0, &sp);
    uint32_t before, total;
    df_bit_offsets(my_bits, wsum, before, total);                  // (`wsum` was last read before many barriers)
    total += hbits;
    if (total + (eob >> 16) < fixed_total) {
        for (uint32_t q = tid; q < (hbits + 31u) >> 5; q += DF_BLK) atomicOr(&img[q], hdr[q]);
        df_tokens<true, DfDyn, DF_WALK_REPLAY>(cd, m, len, in_w, tid, img, hbits + before, &sp);
        if (tid == 0) {
            const uint64_t v = (uint64_t)(eob & 0xffffu) << (total & 31u);
            atomicOr(&img[total >> 5], (uint32_t)v);
            if (v >> 32) atomicOr(&img[(total >> 5) + 1], (uint32_t)(v >> 32));
        }
        total += eob >> 16;
    } else {
        df_tokens<true, DfFixed, DF_WALK_REPLAY>(DfFixed{}, m, len, in_w, tid, img, 3 + fixed_before, &sp);
        if (tid == 0) atomicOr(&img[0], 2u);
        total = fixed_total;
    }
    const uint32_t nbytes = df_marker(img, total);
    if (tid == 0) sizes[c] = nbytes;
    df_store(img, nbytes, slots, c);
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

template <class KERNEL>
static int df_launch(pca_ctx *ctx, KERNEL chunk_kernel, const void *src, const pca_deflate_chunk *chunk_table, int64_t n_chunks, void *out,
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
        hipLaunchKernelGGL(chunk_kernel, dim3((unsigned)n_chunks), dim3(DF_BLK), 0, s, static_cast<const uint8_t *>(src), chunk_table,
                           slots, out_sizes, out_crcs);
        hipLaunchKernelGGL(deflate_offsets, dim3(1), dim3(DF_BLK), 0, s, out_sizes, (int)n_chunks, offs);
        hipLaunchKernelGGL(deflate_compact, dim3((unsigned)n_chunks), dim3(DF_BLK), 0, s, slots, out_sizes, offs, static_cast<uint8_t *>(out));
        PCA_CHECK(ctx, hipGetLastError());
    }
    return pca_side_ticket(ctx);
}

extern "C" int pca_deflate_chunks(pca_ctx *ctx, const void *src, const pca_deflate_chunk *chunk_table, int64_t n_chunks, void *out,
                                  uint32_t *out_sizes, uint32_t *out_crcs, void *workspace, void *stream)
{
    return df_launch(ctx, deflate_chunks, src, chunk_table, n_chunks, out, out_sizes, out_crcs, workspace, stream);
}

extern "C" int pca_deflate_chunks_dyn(pca_ctx *ctx, const void *src, const pca_deflate_chunk *chunk_table, int64_t n_chunks, void *out,
                                      uint32_t *out_sizes, uint32_t *out_crcs, void *workspace, void *stream)
{
    return df_launch(ctx, deflate_chunks_dyn, src, chunk_table, n_chunks, out, out_sizes, out_crcs, workspace, stream);
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
