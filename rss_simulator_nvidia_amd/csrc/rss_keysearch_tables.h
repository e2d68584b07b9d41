// rss_keysearch_tables.h -- what the key-search kernel files share beyond rss_kernel_common.h
// (internal, not ABI): the 8-byte table sets of the search kernels (packed small tables, wide
// pair tables; described in rss_keysearch.hip), the neighbourhood's per-tuple flip span
// (rss_neighbourhood.hip) with its IPv6 tables and span, the u64 load rows and the launch-grid
// rules.  Used by rss_keysearch.hip, rss_neighbourhood.hip, rss_byte_neighbourhood.hip,
// rss_keysearch_weighted.hip, rss_timeline.hip, rss_backlog.hip and rss_symmetric.hip; anonymous
// namespace, as
// rss_kernel_common.h.
#pragma once

#include "rss_kernel_common.h"

namespace {

constexpr uint32_t kPairLutBytes = kSmallTables * 256;            // 5376 (packed kernel)
constexpr uint32_t kPackedBinBytesMax = kLdsBytes - kPairLutBytes;  // 154.75 KiB for the bins
constexpr uint32_t kWidePairLutBytes = 6 * 16384 + 3 * 8192;     // 122880 (pair kernel)
constexpr uint32_t kWidePairBinBytesMax = kLdsBytes - kWidePairLutBytes;  // 40 KiB, 2 x Q bins
constexpr uint32_t kPackedPrepBytes = RSS_INPUT_BITS * 8;  // packed windows, before the bins

__host__ __device__ constexpr int wide_pair_width(int t) {
    return (t == 3 || t == 4 || t == 8) ? 10 : 11;
}
__host__ __device__ constexpr uint32_t wide_pair_table(int t) {  // byte offset
    return t == 0 ? 0u : t == 1 ? 16384u : t == 2 ? 32768u : t == 3 ? 49152u : t == 4 ? 57344u
         : t == 5 ? 65536u : t == 6 ? 81920u : t == 7 ? 98304u : 114688u;
}
// input bit (0 = MSB of the source ip) feeding bit b of table t's index
__host__ __device__ constexpr int wide_pair_bit(int t, int b) {
    return t == 0 ? 31 - b : t == 1 ? 20 - b : t == 2 ? 63 - b
         : t == 3 ? (b < 5 ? 84 - b : 73 - b)
         : t == 4 ? 9 - b : t == 5 ? 52 - b : t == 6 ? 95 - b : t == 7 ? 79 - b : 41 - b;
}

template <int kT>
__device__ __forceinline__ void build_wide_pair_table(uint2* lut, const uint32_t* __restrict__ wa,
                                                      const uint32_t* __restrict__ wb, uint32_t tid) {
    uint32_t a = 0, b = 0;
#pragma unroll
    for (int j = 0; j < 10; ++j) {
        const bool set = (tid >> j) & 1u;
        a ^= set ? wa[wide_pair_bit(kT, j)] : 0u;
        b ^= set ? wb[wide_pair_bit(kT, j)] : 0u;
    }
    uint2* dst = lut + wide_pair_table(kT) / 8;
    dst[tid] = make_uint2(a, b);
    if constexpr (wide_pair_width(kT) == 11)
        dst[tid + 1024] = make_uint2(a ^ wa[wide_pair_bit(kT, 10)], b ^ wb[wide_pair_bit(kT, 10)]);
}

// the nine wide tables of keys (wa, wb), one entry (two for the 11-bit tables) per thread
__device__ __forceinline__ void build_wide_pair_lut(uint2* lut, const uint32_t* __restrict__ wa,
                                                    const uint32_t* __restrict__ wb, uint32_t tid) {
    build_wide_pair_table<0>(lut, wa, wb, tid);
    build_wide_pair_table<1>(lut, wa, wb, tid);
    build_wide_pair_table<2>(lut, wa, wb, tid);
    build_wide_pair_table<3>(lut, wa, wb, tid);
    build_wide_pair_table<4>(lut, wa, wb, tid);
    build_wide_pair_table<5>(lut, wa, wb, tid);
    build_wide_pair_table<6>(lut, wa, wb, tid);
    build_wide_pair_table<7>(lut, wa, wb, tid);
    build_wide_pair_table<8>(lut, wa, wb, tid);
}

// byte address of wide table t's entry: 2 VALU (4 for the two-field t3); tables 5..8 take
// their 64 KiB base from the opaque register `hi`
template <int kT>
__device__ __forceinline__ uint32_t wide_pair_offset(uint32_t w0, uint32_t w1, uint32_t w2,
                                                     uint32_t hi) {
    if constexpr (kT == 0) return (w0 << 3) & 0x3FF8u;
    if constexpr (kT == 1) return (w0 >> 8) & 0x3FF8u;
    if constexpr (kT == 2) return (w1 << 3) & 0x3FF8u;
    if constexpr (kT == 3) return ((w2 >> 8) & 0xF8u) | ((w2 >> 19) & 0x1F00u);
    if constexpr (kT == 4) return (w0 >> 19) & 0x1FF8u;
    if constexpr (kT == 5) return ((w1 >> 8) & 0x3FF8u) | hi;
    if constexpr (kT == 6) return ((w2 << 3) & 0x3FF8u) | hi;
    if constexpr (kT == 7) return ((w2 >> 13) & 0x3FF8u) | hi;
    return ((w1 >> 19) & 0x1FF8u) | hi;
}

template <int kT>
__device__ __forceinline__ uint2 wide_pair_term(const char* lut, uint32_t w0, uint32_t w1,
                                                uint32_t w2, uint32_t hi) {
    constexpr uint32_t kImm = wide_pair_table(kT) & 0xFFFFu;
    return *reinterpret_cast<const uint2*>(lut + kImm + wide_pair_offset<kT>(w0, w1, w2, hi));
}

// (hash under key A, hash under key B) of one tuple on the wide tables
__device__ __forceinline__ uint2 toeplitz_hash_wide_pair(const uint2* __restrict__ lut, uint32_t w0,
                                                         uint32_t w1, uint32_t w2, uint32_t hi) {
    const char* base = reinterpret_cast<const char*>(lut);
    const uint2 t0 = wide_pair_term<0>(base, w0, w1, w2, hi), t1 = wide_pair_term<1>(base, w0, w1, w2, hi);
    const uint2 t2 = wide_pair_term<2>(base, w0, w1, w2, hi), t3 = wide_pair_term<3>(base, w0, w1, w2, hi);
    const uint2 t4 = wide_pair_term<4>(base, w0, w1, w2, hi), t5 = wide_pair_term<5>(base, w0, w1, w2, hi);
    const uint2 t6 = wide_pair_term<6>(base, w0, w1, w2, hi), t7 = wide_pair_term<7>(base, w0, w1, w2, hi);
    const uint2 t8 = wide_pair_term<8>(base, w0, w1, w2, hi);
    return make_uint2(xor3(xor3(t0.x, t1.x, t2.x), xor3(t3.x, t4.x, t5.x), xor3(t6.x, t7.x, t8.x)),
                      xor3(xor3(t0.y, t1.y, t2.y), xor3(t3.y, t4.y, t5.y), xor3(t6.y, t7.y, t8.y)));
}

// entry e = 32 t + v of the 21 pair tables: (XOR of key A's windows, of key B's) over the
// input bits set in v; `win(i)` gives the two keys' window i as a uint2
template <typename Win>
__device__ __forceinline__ void build_small_pair_lut(uint2* lut, Win win, uint32_t tid) {
    for (uint32_t e = tid; e < kSmallLutDwords; e += kBlock) {
        const int t = (int)(e >> 5);
        const uint32_t v = e & 31u;
        const int width = small_width(t % kSmallFields);
        uint32_t a = 0, b = 0;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            if (j < width && ((v >> j) & 1u)) {
                const uint2 w = win(small_slice_bit(t, j));
                a ^= w.x;
                b ^= w.y;
            }
        }
        lut[e] = (v >> width) ? make_uint2(0u, 0u) : make_uint2(a, b);
    }
}

// table 7k + j's 8-byte term for word w (= word k): the field moved to byte offset 8 * field
template <int kT>
__device__ __forceinline__ uint2 small_pair_term(const char* lut, uint32_t w) {
    constexpr int j = kT % kSmallFields, o = 5 * j;
    uint32_t off;
    if constexpr (j == 0)
        off = (w << 3) & 0xF8u;
    else if constexpr (j == 6)
        off = (w >> 27) & 0x18u;
    else
        off = (w >> (o - 3)) & 0xF8u;
    return *reinterpret_cast<const uint2*>(lut + kT * 256 + off);
}

template <int kBase>
__device__ __forceinline__ uint2 small_pair_word(const char* lut, uint32_t w) {  // 7 terms
    const uint2 t0 = small_pair_term<kBase + 0>(lut, w), t1 = small_pair_term<kBase + 1>(lut, w);
    const uint2 t2 = small_pair_term<kBase + 2>(lut, w), t3 = small_pair_term<kBase + 3>(lut, w);
    const uint2 t4 = small_pair_term<kBase + 4>(lut, w), t5 = small_pair_term<kBase + 5>(lut, w);
    const uint2 t6 = small_pair_term<kBase + 6>(lut, w);
    return make_uint2(xor3(xor3(t0.x, t1.x, t2.x), xor3(t3.x, t4.x, t5.x), t6.x),
                      xor3(xor3(t0.y, t1.y, t2.y), xor3(t3.y, t4.y, t5.y), t6.y));
}

// (hash under key A, hash under key B) of one tuple (packed kernel: 8 / 4 keys' low bits)
__device__ __forceinline__ uint2 toeplitz_hash_pair(const uint2* __restrict__ lut, uint32_t w0,
                                                    uint32_t w1, uint32_t w2) {
    const char* base = reinterpret_cast<const char*>(lut);
    const uint2 a = small_pair_word<0>(base, w0), b = small_pair_word<7>(base, w1);
    const uint2 c = small_pair_word<14>(base, w2);
    return make_uint2(xor3(a.x, b.x, c.x), xor3(a.y, b.y, c.y));
}

// ----------------------------------------------------- u64 load bins (weighted, symmetric) --
using u64 = unsigned long long;
constexpr uint32_t kLoadRowBytes = kBinCols * 8;  // one (queue, key)'s columns: the 64 banks once
static_assert(kLoadRowBytes == 256, "a row of u64 columns covers the LDS banks exactly once");

// sum of row e's 32 lane columns (rows of 32 u64 from `bins`), started at column e
__device__ __forceinline__ u64 row_sum(const u64* bins, uint32_t e) {
    u64 s = 0;
    for (uint32_t c = 0; c < kBinCols; ++c) s += bins[e * kBinCols + ((c + e) & (kBinCols - 1))];
    return s;
}

// search kernels' workgroups along x: ~256K tuples per workgroup amortise its 120 KiB table build
inline unsigned search_grid_x(size_t n, int cu_count) {
    const uint64_t slices = (n + (1u << 18) - 1) >> 18;
    return (unsigned)(slices < (uint64_t)cu_count ? slices : cu_count);
}

// --------------------------------------------------------------- neighbourhood --
constexpr uint32_t kNbrBinBytesMax = kLdsBytes - kSmallLutBytes;                  // 161152

// the largest power of two <= 32 of neighbours whose bins fit `budget`
inline uint32_t neighbours_per_workgroup(uint64_t bytes_per_neighbour,
                                         uint32_t budget = kNbrBinBytesMax) {
    uint32_t ng = 32;
    while (ng > 1 && bytes_per_neighbour * ng > budget) ng >>= 1;
    return ng;
}

__device__ __forceinline__ uint32_t alignbit(uint32_t hi, uint32_t lo, uint32_t s) {
    return __builtin_amdgcn_alignbit(hi, lo, s);  // low word of {hi, lo} >> (s & 31)
}

// bits [32 word + s0, 32 word + s0 + 64) of R for one tuple: neighbour j0 + k's delta is the
// low word of this span >> k  (s0 + k <= 31)
__device__ __forceinline__ uint2 flip_span(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t word,
                                           uint32_t s0) {
    const uint32_t x0 = __brev(w0), x1 = __brev(w1), x2 = __brev(w2);
    // R = X << 31 as words r0 .. r3 (r4 = 0)
    const uint32_t r0 = x0 << 31, r1 = alignbit(x1, x0, 1), r2 = alignbit(x2, x1, 1), r3 = x2 >> 1;
    uint32_t lo, hi;
    switch (word) {  // uniform
        case 0: lo = r0; hi = r1; break;
        case 1: lo = r1; hi = r2; break;
        case 2: lo = r2; hi = r3; break;
        default: lo = r3; hi = 0u; break;
    }
    return make_uint2(alignbit(hi, lo, s0), hi >> s0);
}

// IPv6 neighbourhoods (rss_neighbourhood.hip, rss_byte_neighbourhood.hip): nine words
constexpr int kWords6 = RSS_INPUT6_BITS / 32;                                     // 9
template <int kWords>
constexpr uint32_t kNbrLutDwords = kWords * kSmallFields * 32;                    // 672 / 2016
constexpr uint32_t kNbr6BinBytesMax = kLdsBytes - kNbrLutDwords<kWords6> * 4;     // 155776
static_assert(kNbrLutDwords<3> == kSmallLutDwords && kNbr6BinBytesMax == 155776, "table sizes");

// IPv6: the same span from nine words.  With x[-1] = x[9] = x[10] = 0, R's word k is
// alignbit(x[k], x[k - 1], 1) for every k = 0 .. 10, so the span's two words need x[word - 1],
// x[word], x[word + 1] -- a uniform pick among the lane's nine registers (27 v_cndmask_b32).
__device__ __forceinline__ uint2 flip_span6(const uint32_t* w, uint32_t word, uint32_t s0) {
    // selects on scalar conditions (a switch would turn into indexing and put w[] in scratch)
    uint32_t a = 0u, b = 0u, c = 0u;  // tuple words word - 1, word, word + 1 (0 outside the tuple)
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)kWords6; ++k) {
        a = word == k + 1 ? w[k] : a;
        b = word == k ? w[k] : b;
        c = word + 1 == k ? w[k] : c;
    }
    const uint32_t xa = __brev(a), xb = __brev(b), xc = __brev(c);
    const uint32_t lo = alignbit(xb, xa, 1), hi = alignbit(xc, xb, 1);
    return make_uint2(alignbit(hi, lo, s0), hi >> s0);
}

// the 63 IPv6 small tables from the key's ten words (key bits [32 k, 32 k + 32) in kw[k], bit
// 319 unused): window i = key bits [i, i + 32)
__device__ __forceinline__ void build_small_lut6(uint32_t* lut, const uint32_t* __restrict__ kw,
                                                 uint32_t tid) {
    for (uint32_t e = tid; e < kNbrLutDwords<kWords6>; e += kBlock) {
        const int t = (int)(e >> 5);
        const uint32_t v = e & 31u;
        const int width = small_width(t % kSmallFields);
        uint32_t x = 0;
#pragma unroll
        for (int b = 0; b < 5; ++b) {
            const uint32_t i = (uint32_t)small_slice_bit(t, b);  // < 288
            const uint64_t two = (uint64_t)kw[i >> 5] << 32 | kw[(i >> 5) + 1];
            x ^= (b < width && ((v >> b) & 1u)) ? (uint32_t)((two << (i & 31u)) >> 32) : 0u;
        }
        lut[e] = (v >> width) ? 0u : x;
    }
}

__device__ __forceinline__ uint32_t toeplitz_hash_small6(const uint32_t* __restrict__ lut,
                                                         const uint32_t* w) {
    const char* b = reinterpret_cast<const char*>(lut);
    return xor3(xor3(small_word<0>(b, w[0]), small_word<7>(b, w[1]), small_word<14>(b, w[2])),
                xor3(small_word<21>(b, w[3]), small_word<28>(b, w[4]), small_word<35>(b, w[5])),
                xor3(small_word<42>(b, w[6]), small_word<49>(b, w[7]), small_word<56>(b, w[8])));
}

// Neighbourhood workgroups along x.  A workgroup's fixed cost is its bins: q * ng * 32 bins
// cleared and summed again by 1024 lanes, q * ng / 16 LDS accesses per lane, against ng adds per
// tuple -- so q / 2 tuples per lane (at least 16: four 4-tuple loads) keep it near a tenth of
// the work.  That is far less than the search kernels' 256K tuples per workgroup (their 120 KiB
// table build), and 2^20 tuples already fill the device: 64 x 4 workgroups at Q = 24.  No more
// than one round of workgroups (cu_count / y), since each may hold a CU's whole LDS.
inline unsigned neighbourhood_grid_x(size_t n, uint32_t q_eff, unsigned gy, int cu_count) {
    const uint64_t per_wg = (uint64_t)kBlock * std::max<uint32_t>(16u, q_eff / 2);
    const uint64_t slices = (n + per_wg - 1) / per_wg;
    const uint64_t cap = std::max<uint64_t>(1, (uint64_t)cu_count / gy);
    return (unsigned)std::min(slices, cap);
}

}  // namespace
